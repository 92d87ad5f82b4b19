// tsh_block.h -- the candidate block: what the kernels write, the host finalises and the ranks all-gather.
// Plain structs and host arithmetic, no HIP: included by the kernels (tsh_kernels.hip.h), by the finaliser
// (tsh_finalize.h) and, through that one, by tests/cpp/finalize_test.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>

namespace tsh {

// ---------------------------------------------------------------------------
// candidate block written by K2/K3/K4 and shipped to the host (and all-gathered
// between ranks): 64-byte header + entries x {int64 id, f64 s0, f64 s1}
struct BlockHeader {
  uint32_t count;      // candidates found (may exceed `entries`: overflow)
  uint32_t entries;    // capacity of this block
  uint32_t tau_key;    // k-th smallest tile minimum
  uint32_t band_key;   // tau widened by the f32 error band
  uint32_t tiles_hit;  // tiles re-read by K2
  uint32_t flags;      // bit0: K2 list overflow (K3 fallback needed)
  uint32_t k;
  uint32_t metric;
  int64_t row_base;
  int64_t shard_rows;
  uint32_t pad[4];     // [0]: a failed rank's status (FLAG_RANK_ERROR); [1]: the block's generation (sharded calls)
};
static_assert(sizeof(BlockHeader) == 64, "header is 64 bytes");
struct BlockEntry {
  int64_t id;
  double s0;  // L2: sum (q-v)^2   IP: sum q*v   cosine: sum q*v
  double s1;  // cosine: sum v*v   else 0
};
static_assert(sizeof(BlockEntry) == 24, "entry is 24 bytes");
constexpr uint32_t FLAG_LIST_OVERFLOW = 1u;
constexpr uint32_t FLAG_TAU_REFINED = 2u;  // informational: select step (f) ran
constexpr uint32_t FLAG_TAU_UNVERIFIED = 4u;  // batched path: the estimated filter threshold was too tight (set with
                                              // FLAG_LIST_OVERFLOW: the query is redone by the single-query path)

// candidate entries as the finaliser takes them, from any number of blocks (tsh_finalize.h)
typedef std::pair<const BlockEntry *, uint32_t> EntryList;
// a block's own: the entries behind its header, as many as it holds (an overflowed block holds `entries` of `count`)
inline EntryList block_list(const uint8_t *block) {
  const BlockHeader *h = reinterpret_cast<const BlockHeader *>(block);
  return {reinterpret_cast<const BlockEntry *>(block + sizeof(BlockHeader)), std::min(h->count, h->entries)};
}

}  // namespace tsh
