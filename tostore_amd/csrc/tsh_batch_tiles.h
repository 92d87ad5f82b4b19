// tsh_batch_tiles.h -- which (query tile, row tile) workgroup slot b of a batched key pass scores.  Integer arithmetic
// only, no HIP: the key kernels reach it through batch_tile_of(const BatchArgs &, ...) (tsh_batch.hip.h), and
// tests/cpp/batch_tiles_test.cpp compiles it on its own with g++.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSH_TILES_FN __host__ __device__ __forceinline__
#else
#define TSH_TILES_FN inline
#endif

namespace tsh {

// XCD-aware tile order: workgroup b runs on XCD b % 8; give each XCD runs of
// q_tiles consecutive workgroups that share one row tile (L2 reuse of V)
TSH_TILES_FN void batch_tile_of(int q_tiles, int n_tiles, int b, int *q_tile, int *n_tile) {
  const int total = q_tiles * n_tiles;
  const int xcd = b & 7, i = b >> 3;
  const int per_round = 8 * q_tiles;
  const int full_rounds = total / per_round;
  if (b < full_rounds * per_round) {
    *q_tile = i % q_tiles;
    *n_tile = (i / q_tiles) * 8 + xcd;
  } else {  // ragged tail: plain order
    int r = b - full_rounds * per_round;
    *n_tile = full_rounds * 8 + r / q_tiles;
    *q_tile = r % q_tiles;
  }
}

}  // namespace tsh
