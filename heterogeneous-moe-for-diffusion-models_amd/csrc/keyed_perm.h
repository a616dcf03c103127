// Keyed permutation of [0, N): the epoch order of the device-resident dataset (contract in include/hdmoe.h, "keyed permutation").
// One definition for the per-sample kernel of csrc/traingen.hip and the host entry point hdmoe_dataset_perm, so that the host can
// say which items a step holds without a device and the two agree by construction.
//
// A balanced Feistel network over k = 2h bits (k = the even bit length of N - 1, at least 2) is a bijection of [0, 2^k) whatever its
// round function is; walking its cycle from a point inside [0, N) until it re-enters [0, N) restricts it to a bijection of [0, N)
// (2^k < 4 N + 4, so the expected walk is under four applications).  Round function: word 0 of the Philox4x32-10 block (R, round)
// under the (seed, epoch) key.  Eight rounds: with four, single positions of small N are visibly non-uniform over the epochs.
#pragma once
#include "common.h"

constexpr int KPERM_ROUNDS = 8;

struct KeyedPerm {
  uint32_t k0, k1, N, m;
  int h;
};

HDI KeyedPerm keyed_perm_make(unsigned long long seed, unsigned long long epoch, uint32_t N) {
  int bits = 0;
  while (bits < 32 && ((N - 1u) >> bits)) ++bits;           // bit_length(N - 1); N < 2^31 keeps it <= 31
  int k = bits < 2 ? 2 : bits;
  k += k & 1;
  const unsigned long long K = (seed ^ 0xA0761D6478BD642Full) + epoch * 0x9E3779B97F4A7C15ull;
  KeyedPerm p;
  p.k0 = (uint32_t)K; p.k1 = (uint32_t)(K >> 32); p.N = N; p.h = k >> 1; p.m = (1u << (k >> 1)) - 1u;
  return p;
}

// perm(x) for 0 <= x < N
HDI uint32_t keyed_perm_at(const KeyedPerm& p, uint32_t x) {
  uint32_t y = x;
  do {
    uint32_t L = y >> p.h, R = y & p.m;
    for (int r = 0; r < KPERM_ROUNDS; ++r) {
      uint32_t o[4];
      philox(R, (uint32_t)r, p.k0, p.k1, o);
      const uint32_t t = L ^ (o[0] & p.m);
      L = R; R = t;
    }
    y = (L << p.h) | R;
  } while (y >= p.N);
  return y;
}
