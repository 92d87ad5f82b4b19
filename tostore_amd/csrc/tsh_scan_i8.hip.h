// tsh_scan_i8.hip.h -- what follows the coarse int8 scan (scan_i8_kernel, tsh_kernels.hip.h) on the way to the exact
// path (gfx950, wave = 64).  The scan left per row the LOWER side of its key's band and per tile two minima: of the
// UPPER sides (gmin[t]) and, behind those, of the LOWER sides (gmin[n_tiles + t]).  One launch turns them into the list:
//   L  i8_list_kernel       one workgroup.  tau = the k-th smallest upper minimum (select_tau: steps (a)-(c) of K2).  k
//                           distinct tiles hold a row whose exact key is <= tau, so the top k all have a lower side
//                           <= tau.  Fewer than k live tiles: tau = KEY_NAN, every live row survives.  (A masked
//                           scan's dead tiles hold KEY_DEAD, the largest key, in both minima: select_tau never counts
//                           them towards k and nothing below looks at their stale keys[].)
//                           A tile whose lower minimum is above tau holds no survivor: only the others -- a few hundred
//                           of a 1 M-row shard's 15 625 -- have their 64 keys read again and balloted against tau, and
//                           the ballots' set bits go out as the ASCENDING id list the exact path needs (position is its
//                           tie-break), capped and padded to I8_LIST_CAP entries, with the survivors' total next to it.
// E1 + E2 / E2' (tsh_exact.hip.h) then run over those I8_LIST_CAP entries -- padding entries are dead -- and write the
// block; a total above the capacity raises FLAG_LIST_OVERFLOW | FLAG_I8_OVERFLOW in its header and the host redoes the
// query through the f32 scan.  More than I8_LIST_CAP candidate TILES are such an overflow by themselves (each holds a
// survivor): the total is then their number and the list all padding.
#pragma once

#include "tsh_kernels.hip.h"

namespace tsh {

constexpr int I8_LIST_CAP = 4096;  // survivors the exact path takes: ~8x what a 1 M x 768 corpus leaves at k = 100
// candidate tiles per wave and round: their key loads are all in flight at once (a round is a trip to memory; 16 waves x
// 32 take the headline's ~400 candidate tiles in one)
constexpr int I8_LIST_TILES = 32;
static_assert(I8_LIST_CAP <= SEL_LIST_CAP, "the candidate tiles' ids live in select_tau's list");
static_assert(I8_LIST_CAP % SEL_THREADS == 0, "a whole number of candidate tiles per thread");

// ctl[0] = tau, ctl[1] = the survivors' total (above I8_LIST_CAP: an overflow); list[0 .. I8_LIST_CAP): their ids,
// ascending, then 0xFFFFFFFF.  lo = gmin + n_tiles: the tiles' minima of lower sides.
template <bool IN_REGS>
__global__ void __launch_bounds__(SEL_THREADS) i8_list_kernel(const uint32_t *gmin, const uint32_t *keys, int32_t n_tiles, int32_t k,
                                                              uint32_t *__restrict__ list, uint32_t *__restrict__ ctl) {
  constexpr int NW = SEL_THREADS / 64, CPT = I8_LIST_CAP / SEL_THREADS;
  __shared__ SelectTauLds<SEL_THREADS> s_t;
  __shared__ uint64_t s_word[I8_LIST_CAP];  // a candidate tile's ballot of keys <= tau
  __shared__ uint32_t s_wsum[2][NW];        // the waves' totals: [0] of candidate tiles, [1] of survivors
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t *lo = gmin + n_tiles;
  const uint64_t below = (1ull << lane) - 1ull;
  // candidate tiles, ascending: a wave takes a contiguous run of `per` x 64 tiles, 64 at a time -- its ballots order
  // them without a barrier -- and one scan of the sixteen wave totals places the runs
  const int per = (n_tiles + SEL_THREADS - 1) / SEL_THREADS;  // (IN_REGS: <= SEL_VPT)
  const int t0 = wave * per * 64 + lane;
  uint32_t v[SEL_VPT];
  if (IN_REGS) {  // (the lower minima are on their way while the threshold is found)
#pragma unroll
    for (int i = 0; i < SEL_VPT; ++i) {
      const int t = t0 + i * 64;
      v[i] = i < per && t < n_tiles ? lo[t] : KEY_DEAD;
    }
  }
  {
    uint32_t g[SEL_VPT];
    select_tau<SEL_THREADS, IN_REGS>(gmin, n_tiles, (uint32_t)k, false, g, s_t);
  }
  const uint32_t tau = s_t.tau;  // (<= KEY_NAN < KEY_DEAD: no dead tile is a candidate, no absent row survives)
  uint32_t n_mine = 0;  // wave-uniform
  if (IN_REGS) {
#pragma unroll
    for (int i = 0; i < SEL_VPT; ++i) n_mine += (uint32_t)__popcll(__ballot(v[i] <= tau));
  } else {
    for (int i = 0; i < per; ++i) {
      const int t = t0 + i * 64;
      n_mine += (uint32_t)__popcll(__ballot(t < n_tiles && lo[t] <= tau));
    }
  }
  if (lane == 0) s_wsum[0][wave] = n_mine;
  __syncthreads();
  uint32_t pos = 0, n_cand = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t x = s_wsum[0][i];
    if (i < wave) pos += x;
    n_cand += x;
  }
  const bool over = n_cand > (uint32_t)I8_LIST_CAP;  // workgroup-uniform
  if (!over) {
    if (IN_REGS) {
#pragma unroll
      for (int i = 0; i < SEL_VPT; ++i) {
        const bool hit = v[i] <= tau;
        const uint64_t b = __ballot(hit);
        if (hit) s_t.list[pos + (uint32_t)__popcll(b & below)] = (uint32_t)(t0 + i * 64);
        pos += (uint32_t)__popcll(b);
      }
    } else {
      for (int i = 0; i < per; ++i) {
        const int t = t0 + i * 64;
        const bool hit = t < n_tiles && lo[t] <= tau;
        const uint64_t b = __ballot(hit);
        if (hit) s_t.list[pos + (uint32_t)__popcll(b & below)] = (uint32_t)t;
        pos += (uint32_t)__popcll(b);
      }
    }
  }
  __syncthreads();
  const uint32_t nc = over ? 0u : n_cand;

  // the candidate tiles' ballots: I8_LIST_TILES tiles per wave and round
  for (uint32_t j0 = (uint32_t)wave * I8_LIST_TILES; j0 < nc; j0 += NW * I8_LIST_TILES) {
    uint32_t key[I8_LIST_TILES];
#pragma unroll
    for (int u = 0; u < I8_LIST_TILES; ++u) key[u] = j0 + u < nc ? keys[(int64_t)s_t.list[j0 + u] * 64 + lane] : KEY_DEAD;
    uint64_t mine = 0;
#pragma unroll
    for (int u = 0; u < I8_LIST_TILES; ++u) {
      const uint64_t b = __ballot(key[u] <= tau);
      if (lane == u) mine = b;
    }
    if (lane < I8_LIST_TILES && j0 + lane < nc) s_word[j0 + lane] = mine;
  }
  __syncthreads();

  // the list: a thread owns CPT consecutive candidate tiles; its first position = the survivors in front of it
  uint64_t word[CPT];
  uint32_t c = 0;
#pragma unroll
  for (int u = 0; u < CPT; ++u) {
    const uint32_t j = (uint32_t)(tid * CPT + u);
    word[u] = j < nc ? s_word[j] : 0ull;
    c += (uint32_t)__popcll(word[u]);
  }
  uint32_t incl = c;  // inclusive prefix within the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += x;
  }
  if (lane == 63) s_wsum[1][wave] = incl;
  __syncthreads();
  uint32_t o = incl - c, total = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t x = s_wsum[1][i];
    if (i < wave) o += x;
    total += x;
  }
#pragma unroll
  for (int u = 0; u < CPT; ++u) {
    if (!word[u]) continue;
    const uint32_t base = s_t.list[tid * CPT + u] * 64u;
    // (ids past the capacity are counted, not written)
    for (uint64_t w = word[u]; w; w &= w - 1, ++o)
      if (o < (uint32_t)I8_LIST_CAP) list[o] = base + (uint32_t)__builtin_ctzll(w);
  }
  for (uint32_t i = total + (uint32_t)tid; i < (uint32_t)I8_LIST_CAP; i += SEL_THREADS) list[i] = 0xFFFFFFFFu;
  if (tid == 0) {
    ctl[0] = tau;
    ctl[1] = over ? n_cand : total;
  }
}

}  // namespace tsh
