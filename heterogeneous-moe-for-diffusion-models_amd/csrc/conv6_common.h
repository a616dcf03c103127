// Shared by the conv6-class kernels (conv6, conv6s, blk6; conv7 takes the epilogue pack): launch arguments and work-unit record of conv6 / conv6s,
// the device helpers every body uses and the plan helpers of conv6_plan / conv6s_plan.
#pragma once
#include "conv_args.h"

namespace {

typedef __attribute__((address_space(3))) void* lptr_t;

struct C6Args {
  const void* x; const void* w; void* y; const void* res; const int* seg;
  long wstride;                       // elements per group in the weight image [g][tap][Cout][Cin]
  int N, H, W, Cin, Cout, ngroups;
  int ks[HDMOE_MAX_GROUPS], pt[HDMOE_MAX_GROUPS], pl[HDMOE_MAX_GROUPS], order[HDMOE_MAX_GROUPS];
  float alpha, beta;
  int TH, TW, tws, tiles_x, tpi;      // tile geometry (TW = 1 << tws), tiles per image
  int T;                              // taps per weight stage
  int nblk;                           // output-channel blocks
  int hb_bytes, wb_bytes;             // bytes of one halo buffer / one weight buffer
  int xbytes, wbytes;                 // extents of x and of the weight image (buffer descriptors; < 4 GB)
  unsigned ybytes;                    // extent of y for buffer-descriptor stores with a counted drain (conv6_body.h epilogue); 0: plain stores
  unsigned m_nblk, m_T, m_tpi, m_tx;  // 2^32 / d + 1 reciprocals of nblk, T, tpi, tiles_x
  int w_rowpitch, w_tapstride;        // weight image geometry in elements: between consecutive output rows / consecutive taps (default Cin, Cout * Cin);
                                      // larger values read a [tap][rows][pitch] image with more channels / rows than this conv uses
                                      // (the ones-channel layer of Unet_expert: hdmoe_conv6_ones_fwd / _bwd)
  const float* gbias;                 // optional fp32 [group][H][W][Cout]: y = alpha * (acc + gbias[g][yy][xx][:]) + beta * res
  int dbg;                            // always 0.  conv6s_body.h keeps its tests on it: without them the split kernel needs one VGPR more
  unsigned long long* stamps;         // development: s_memtime stamps of workgroup 0 ([wave][64] slots), or null
  // fused FiLM epilogue (Unet_block, reference model_components.py:242-246): besides y the kernel writes
  // film_h = dropout_p(mp_silu(y * film_e[n][c])) -- the same arithmetic and the same Philox bits as film_silu_fwd_kernel<bf16, 8>
  // (elementwise.hip) on the bf16-rounded y, so the separate pass (and its launch on the U-Net branch's serial chain) disappears.
  const float* film_e; void* film_h; const unsigned long long* film_seed_dev; unsigned film_seed_lo, film_seed_hi; float film_p;
};

template <int MT>
struct C6Unit {                       // one work unit: MT 256-pixel tiles of one expert x one output-channel block (all wave-uniform)
  int g, ks, ntaps, ntg, pt, pl, HWp, HHp, ppt, nbk;
  int n[MT], ty0[MT], tx0[MT], valid[MT];
};

constexpr int C6_MAXT = 9;            // taps per weight stage (<= 9: the stage's tap loop is fully unrolled)
constexpr int C6_NW = 8;              // waves per workgroup: two per SIMD.  (One per SIMD with twice the tile per wave measured 20 % slower: a lone wave
                                      // issues its ~4.5 LDS / VALU / scalar instructions per MFMA in the open, a partner wave hides them.)

#if __HIP_DEVICE_COMPILE__                 // (the lane builtins exist in the device pass only; the bodies that call these are guarded alike)

// x / d for small non-negative x: 32.32 reciprocal (magic = conv_recip(d)) + fix-up
DEVI int c6_udiv(int x, unsigned magic, int d) {
  int q = (int)(((unsigned long long)(unsigned)x * magic) >> 32);
  if (q * d > x) --q;
  if ((q + 1) * d <= x) ++q;
  return q;
}

// The persistent kernels (conv6, conv6s, blk6) keep slot oi of their unit list in lane oi < ngroups of every wave: first unit `ustart` and
// unit count `units` of the slot.  Slot of unit u (wave-uniform: a ballot, no memory access); a u beyond the list lands in slot 7.
DEVI int c6_slot_of(int u, int ustart, int units, int lane) {
  const unsigned long long hit = __ballot((lane < 8) & ((u >= ustart) & (u < ustart + units)));
  return (int)__builtin_ctzll(hit | (1ull << 7));
}

// bf16 epilogue pack.  v: the lane's register quads 2p (channels 16p + 4h ..) and 2p + 1 (channels 16p + 8 + 4h ..) of its pixel.  The
// two swaps pair the quads across the half-waves: the lower half ends up with channels 16p .. 16p + 7, the upper half with
// 16p + 8 .. 16p + 15, as the four words of one 16-byte store at channel 16p + 8h.
struct C6Words { unsigned w[4]; };
DEVI C6Words c6_pack_bf16(const float (&v)[8]) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  const unsigned A0 = __builtin_bit_cast(unsigned, (bf2){(bf16)v[0], (bf16)v[1]}), A1 = __builtin_bit_cast(unsigned, (bf2){(bf16)v[2], (bf16)v[3]});
  const unsigned B0 = __builtin_bit_cast(unsigned, (bf2){(bf16)v[4], (bf16)v[5]}), B1 = __builtin_bit_cast(unsigned, (bf2){(bf16)v[6], (bf16)v[7]});
  const u32x2 s0 = __builtin_amdgcn_permlane32_swap(A0, B0, false, false);
  const u32x2 s1 = __builtin_amdgcn_permlane32_swap(A1, B1, false, false);
  return C6Words{{s0[0], s1[0], s0[1], s1[1]}};
}

// ---- LDS images: lane-linear 1-KB DMA pieces (16 rows x 64 B), 16-byte slot ^= (row >> 2) & 3 on the DMA source and on the fragment read
DEVI int c6_dma_csl(int lane) { return ((lane & 3) ^ ((lane >> 4) & 3)) << 4; }   // byte offset of the (swizzled) 16-B channel slot a DMA lane fetches
DEVI int c6_dma_prow(int lane) { return lane >> 2; }                              // its row inside the piece
DEVI int c6_wfrag_off(int r, int h) { return r * 64 + ((h << 4) ^ (((r >> 2) & 3) << 4)); }   // a lane's weight-fragment byte offset inside a tap block
// a wave's share of a weight stage of ntl taps: piece pi = wave + NW k is tap pi / PPT, rows 16 * (pi % PPT) .. (PPT pieces per tap, NW % PPT == 0)
template <int PPT, int NW> DEVI int c6_wpieces(int ntl, int wave) { return max(0, (ntl - wave / PPT + (NW / PPT) - 1) / (NW / PPT)); }
// row of pixel px inside a halo image of row pitch WP, by a 2^20 reciprocal + fix-up (magic = c6_halo_magic(WP)); the column is px - row * WP
DEVI int c6_halo_magic(int WP) { return (1 << 20) / WP + 1; }
DEVI int c6_halo_row(int px, int magic, int WP) {
  int hy = (int)(((unsigned)px * (unsigned)magic) >> 20);
  if (hy * WP > px) --hy;
  return hy;
}

#endif

}  // namespace

// 256-pixel tile geometry and output-channel blocks of conv6_plan / conv6s_plan; returns NT (32-channel blocks per unit: 2 or 1)
static inline int c6_plan_tiles(const ConvArgs& c, C6Args& a) {
  a.TW = c.W >= 32 ? 32 : 16; a.tws = a.TW == 32 ? 5 : 4; a.TH = 256 / a.TW;
  a.tiles_x = c.W / a.TW;
  a.tpi = a.tiles_x * (int)cdiv(c.H, a.TH);
  const int NT = c.Cout % 64 == 0 ? 2 : 1;
  a.nblk = c.Cout / (32 * NT);
  return NT;
}
static inline void c6_plan_magics(C6Args& a) {
  a.m_nblk = conv_recip(a.nblk); a.m_T = conv_recip(a.T); a.m_tpi = conv_recip(a.tpi); a.m_tx = conv_recip(a.tiles_x);
}

struct C6Plan { C6Args a; int MT, NT; unsigned G; size_t lds; };
// Launch geometry of conv6 for one layer (conv6.hip).  0 = planned, 1 = outside conv6's domain.
int conv6_plan(const ConvArgs& c, int dtype, C6Plan& plan);
