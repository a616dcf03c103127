// Pointwise streaming kernels (lwgrad.hip, pbwd.hip, kgemm.hip, the weight-gradient half of fusion.hip): the one definition of what they
// share.  A wave streams position slices of position-major bf16 tensors through WAVE-PRIVATE LDS sub-tiles ([rows][64 B]), fetches both
// MFMA operands of dW[o][i] = sum_p dy[p][o] x[p][i] back with transposing reads, and the waves of a workgroup meet once, in LDS, before
// one flush.  No class hierarchy: free functions and one register record, in the style of common.h.
#pragma once
#include "common.h"

// ---- partition slot -> (expert g, positions [p0, p1), 64-position slices [u0, u1) of them): every expert takes ceil(slices / upw)
// consecutive slots (one without rows takes none); false past the last expert's last slot
DEVI bool pws_slot(const int* seg, int ngroups, int N, long HW, int upw, int slot, int& g, long& p0, long& p1, long& u0, long& u1) {
  for (g = 0; g < ngroups; ++g) {
    const long r0 = seg ? seg[g] : 0, r1 = seg ? seg[g + 1] : N;
    p0 = r0 * HW; p1 = r1 * HW;
    const long units = (p1 - p0 + 63) >> 6;
    const long nch = (units + upw - 1) / upw;
    if (slot < nch) { u0 = (long)slot * upw; u1 = u0 + upw < units ? u0 + upw : units; return true; }
    slot -= (int)nch;
  }
  return false;
}

// ---- hand-over of a wave-private tile between the wave's own writes and reads: the LDS keeps one wave's accesses in order, so this is
// a compiler fence, not a workgroup barrier (two barriers per slice marched the four waves of lwgrad.hip in lockstep until round 3)
DEVI void pws_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- transposing fragment read: 8 consecutive rows (k) of channel lane & 31 from a [rows][64 B] sub-tile.  Lane (h = lane >> 5, ..)
// reads row pws_tr_row(lane) (+ 4 for the second half) at byte column pws_tr_col(lane); the caller forms the two byte addresses, so a
// swizzled tile (fusion.hip wg_off) is served as well.  The builtin form: these kernels run no LDS-DMA (common.h, lds_tr2_issue).
typedef __attribute__((address_space(3))) hd_s16x4* pws_lds_p4;
DEVI int pws_tr_row(int lane) { return 8 * (lane >> 5) + ((lane & 15) >> 2); }
DEVI int pws_tr_col(int lane) { return 2 * (lane & 16) + 8 * (lane & 3); }
DEVI bf16x8 pws_tr8(const unsigned char* lo4, const unsigned char* hi4) {
  const hd_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pws_lds_p4)(lo4));
  const hd_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pws_lds_p4)(hi4));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- one 64-position slice of dy [P][O] (OT 32-channel sub-tiles from column o0) and x [P][I] (IT sub-tiles from column i0) on its way
// from HBM to the wave's sub-tiles `mine`: dy sub-tiles [OT][64 positions][64 B], then x sub-tiles [IT][64][64 B]
template <int OT, int IT>
struct PwsSlice {
  uint4 sdy[4 * OT], sx[4 * IT];
  // slice at position pb of the range [p0, p1).  DUAL (OT = 2): sub-tile 0 from dy, sub-tile 1 from dy2, both [P][32]
  template <bool DUAL = false>
  DEVI void load(const bf16* DY, const bf16* DY2, const bf16* X, int O, int I, int o0, int i0, long pb, long p0, long p1, int lane) {
    static_assert(!DUAL || OT == 2, "two layers = two output tiles");
#pragma unroll
    for (int k = 0; k < 4 * OT; ++k) {
      const int e = lane + 64 * k, q = e / (4 * OT), pc = e % (4 * OT);
      const long p = pb + q;
      if constexpr (DUAL) sdy[k] = *reinterpret_cast<const uint4*>((pc < 4 ? DY : DY2) + (p < p1 ? p : p0) * 32 + (pc & 3) * 8);
      else sdy[k] = *reinterpret_cast<const uint4*>(DY + (p < p1 ? p : p0) * O + o0 + pc * 8);
    }
#pragma unroll
    for (int k = 0; k < 4 * IT; ++k) {
      const int e = lane + 64 * k, q = e / (4 * IT), pc = e % (4 * IT);
      const long p = pb + q;
      sx[k] = *reinterpret_cast<const uint4*>(X + (p < p1 ? p : p0) * I + i0 + pc * 8);
    }
    // positions past the range were read from the range's first position; they are zeroed here, after ALL loads were issued (a
    // `cond ? load : 0` form serialises the loads behind one another)
#pragma unroll
    for (int k = 0; k < 4 * OT; ++k) if (pb + (lane + 64 * k) / (4 * OT) >= p1) sdy[k] = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 4 * IT; ++k) if (pb + (lane + 64 * k) / (4 * IT) >= p1) sx[k] = make_uint4(0, 0, 0, 0);
  }
  DEVI void store(unsigned char* mine, int lane) const {
#pragma unroll
    for (int k = 0; k < 4 * OT; ++k) {
      const int e = lane + 64 * k, q = e / (4 * OT), pc = e % (4 * OT);
      *reinterpret_cast<uint4*>(mine + (pc >> 2) * 4096 + q * 64 + (pc & 3) * 16) = sdy[k];
    }
#pragma unroll
    for (int k = 0; k < 4 * IT; ++k) {
      const int e = lane + 64 * k, q = e / (4 * IT), pc = e % (4 * IT);
      *reinterpret_cast<uint4*>(mine + OT * 4096 + (pc >> 2) * 4096 + q * 64 + (pc & 3) * 16) = sx[k];
    }
  }
  // acc[t][v] += dy_t^T x_v over the 64 positions staged in `mine`: four 16-position k-steps in order
  static DEVI void mma(const unsigned char* mine, int lane, f32x16 (&acc)[OT][IT]) {
    const int tlane = pws_tr_row(lane) * 64 + pws_tr_col(lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 fdy[OT], fx[IT];
#pragma unroll
      for (int t = 0; t < OT; ++t) { const unsigned char* b = mine + t * 4096 + ks * 1024 + tlane; fdy[t] = pws_tr8(b, b + 4 * 64); }
#pragma unroll
      for (int v = 0; v < IT; ++v) { const unsigned char* b = mine + (OT + v) * 4096 + ks * 1024 + tlane; fx[v] = pws_tr8(b, b + 4 * 64); }
#pragma unroll
      for (int t = 0; t < OT; ++t)
#pragma unroll
        for (int v = 0; v < IT; ++v) acc[t][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fdy[t], fx[v], acc[t][v], 0, 0, 0);
    }
  }
};

// ---- the waves' accumulators meet in LDS: red[(slot * NT + t) * 16 + reg][lane] floats, lane-major so that both the write and the
// summing read are conflict-free.  Element e = (t * 16 + reg) * 64 + lane of a slot's NT tiles is row acc_row(reg, lane), column
// lane & 31 of tile t.  The workgroup barriers around the hand-over are the caller's.
template <int NT>
DEVI void pws_put(float* red, int slot, int lane, const f32x16* acc) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) red[((slot * NT + t) * 16 + reg) * 64 + lane] = acc[t][reg];
}
// element e summed over the slots 0 .. NW - 1, in that order, from 0.f
template <int NW, int NT>
DEVI float pws_sum(const float* red, int e) {
  float v = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) v += red[w * NT * 1024 + e];
  return v;
}
// Every workgroup of a launch adds into the same words: each starts at its own element `rot` (the caller's expression), so that they do
// not all queue on the same addresses at the same time.  dst(tile, reg, lane) is the element's word, or null for one that has none.
// All `nthreads` threads of the workgroup call it.
template <int NW, int NT, typename Dst>
DEVI void pws_flush(const float* red, int tid, int nthreads, int rot, Dst dst) {
  for (int e0 = tid; e0 < NT * 1024; e0 += nthreads) {
    const int e = (e0 + rot) % (NT * 1024);
    const float v = pws_sum<NW, NT>(red, e);
    float* p = dst(e >> 10, (e >> 6) & 15, e & 63);
    if (p) atomicAdd(p, v);
  }
}

// ---- host: the launch of lwgrad.hip's slice kernels over `positions` positions in `ngroups` expert groups, ib x ob tiles of
// [32 * OT][32 * IT] weights; `staged`: the bf16 kernel, whose staged operands share the buffer with the reduction
struct PwsPlan { int upw; dim3 grid; size_t lds; };
static inline bool pws_plan(PwsPlan& p, long positions, int ngroups, long ib, long ob, int OT, int IT, bool staged) {
  const long units = (positions + 63) / 64 + ngroups;                    // 64-position slices (upper bound over the experts' ragged ends)
  long upw = (units * ib * ob + 511) / 512;                              // ~512 workgroups per launch
  if (upw < 4) upw = 4;                                                  // at least one slice per wave
  if (upw > 4096) upw = 4096;
  const long slots = units / upw + ngroups + 1;
  if (slots > 65535 || ob > 65535) return false;
  const size_t red = (size_t)4 * OT * IT * 4096, stage = (size_t)4 * (OT + IT) * 4096;
  p.upw = (int)upw;
  p.grid = dim3((unsigned)ib, (unsigned)ob, (unsigned)slots);
  p.lds = staged && stage > red ? stage : red;
  return true;
}
