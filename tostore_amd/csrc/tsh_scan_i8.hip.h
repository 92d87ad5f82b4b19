// tsh_scan_i8.hip.h -- what follows the coarse int8 scan (scan_i8_kernel, tsh_kernels.hip.h) on the way to the exact
// path (gfx950, wave = 64).  The scan left per row the LOWER side of its key's band and per tile the minimum of the
// UPPER sides:
//   T1 i8_tau_kernel        one workgroup: tau = the k-th smallest tile minimum (select_tau: steps (a)-(c) of K2).  k
//                           distinct tiles hold a row whose exact key is <= tau, so the top k all have a lower side
//                           <= tau.  Fewer than k live tiles: tau = KEY_NAN, every live row survives.  (A masked
//                           scan's dead tiles hold KEY_DEAD, the largest key: select_tau never counts them towards k.)
//   T2 i8_survivor_kernel   a wave per sixteen tiles: one ballot word per tile of keys[i] <= tau (0 for a dead tile of a
//                           masked scan, whose keys[] are stale) -- a row mask like any other, which M1 / M2 (tsh_mask.hip.h) count and compact into the ASCENDING id list the exact
//                           path needs (position is its tie-break), capped and padded to I8_LIST_CAP entries by M2 itself.
// E1 + E2 / E2' (tsh_exact.hip.h) then run over those I8_LIST_CAP entries -- padding entries are dead -- and write the
// block; a survivor count above the capacity (M2's total) raises FLAG_LIST_OVERFLOW | FLAG_I8_OVERFLOW in its header
// and the host redoes the query through the f32 scan.
#pragma once

#include "tsh_kernels.hip.h"

namespace tsh {

constexpr int I8_LIST_CAP = 4096;  // survivors the exact path takes: ~8x what a 1 M x 768 corpus leaves at k = 100

template <bool IN_REGS>
__global__ void __launch_bounds__(SEL_THREADS) i8_tau_kernel(const uint32_t *gmin, int32_t n_tiles, int32_t k, uint32_t *tau_out) {
  __shared__ SelectTauLds<SEL_THREADS> s_t;
  uint32_t g[SEL_VPT];
  select_tau<SEL_THREADS, IN_REGS>(gmin, n_tiles, (uint32_t)k, false, g, s_t);
  if (threadIdx.x == 0) *tau_out = s_t.tau;
}

constexpr int I8_SURV_TILES = 16;  // tiles per wave of T2: their key loads are all in flight at once
static __global__ void __launch_bounds__(256) i8_survivor_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ gmin,
                                                                 const uint32_t *__restrict__ tau_p, int32_t n_tiles,
                                                                 uint64_t *__restrict__ words) {
  const int lane = threadIdx.x & 63;
  const int t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * I8_SURV_TILES;
  if (t0 >= n_tiles) return;  // wave-uniform
  const uint32_t tau = *tau_p;
  // (lane i: is tile t0 + i dead?  A masked scan left such a tile's keys[] as they were; gmin = NULL: a dense scan)
  const bool dead_tile = gmin && lane < I8_SURV_TILES && t0 + lane < n_tiles && gmin[t0 + lane] == KEY_DEAD;
  uint32_t key[I8_SURV_TILES];
#pragma unroll
  for (int i = 0; i < I8_SURV_TILES; ++i) key[i] = t0 + i < n_tiles ? keys[(int64_t)(t0 + i) * 64 + lane] : KEY_DEAD;
  uint64_t mine = 0;
#pragma unroll
  for (int i = 0; i < I8_SURV_TILES; ++i) {
    const uint64_t b = __ballot(key[i] <= tau);  // (tau <= KEY_NAN < KEY_DEAD: no absent row survives)
    if (lane == i) mine = b;
  }
  if (lane < I8_SURV_TILES && t0 + lane < n_tiles) words[t0 + lane] = dead_tile ? 0ull : mine;
}

}  // namespace tsh
