// tsh_batch_f16.hip.h -- what the fp16 pre-filter key kernel of the batched path (TSH_OPT_BATCH_KERNEL = 2 / auto;
// batch_score_f16pp_kernel, tsh_batch_f16pp.hip.h) and the upkeep of its operand planes share: the plane layout and the
// kernel that converts rows into it (half_rows32_kernel), the norm-grouped order of an L2 / inner-product shard's plane
// (plane_group_kernel), the gather of a listed call's norms, and the LDS-DMA helpers.  The key kernel's contract is that
// of batch_score_bf16x3_kernel<MODE = 1> in tsh_batch.hip.h: operands rounded to fp16 after an exact power-of-two
// scaling, ONE v_mfma_f32_32x32x16_f16 per product, key transform + per-query threshold filter fused into the epilogue.
//
//   * operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging registers, no ds_write pass.
//     The DMA writes a wave's 64 x 16 B linearly, so the bank swizzle the fragment reads need is baked into the
//     GLOBAL layout of the planes ("plane32" below): a tile's K-chunk is a contiguous run of 8 KB blocks that are
//     byte for byte the LDS image.
//   * K-chunk = 32 (64 B per row), a ring of four stages; a wave waits for its own DMA pieces with a COUNTED
//     s_waitcnt vmcnt.  The DMA is issued from inline asm, so the compiler's own s_waitcnt insertion does not see it
//     (it would drain it before every LDS read); the counts are kept by hand.
//   * survivors of the filter are collected in a per-wave LDS list of F16_HITS entries without atomics (slot = running
//     scalar count + mbcnt of the hit mask) and flushed once per tile: one returning global atomic per survivor, all
//     in flight together, instead of one wait per hit site.
//
// (The kernel these pieces were first written for -- the second generation: eight waves interleaving reads, DMA issue
// and MFMAs around one barrier per K-step -- is gone: it predated BatchArgs::row_ids, so it could score neither a
// norm-grouped plane nor a listed call.)
//
// Plane layout "plane32": rows in groups of 128; per group and K-chunk of 32 one 8 KB block;
//   16-byte piece(row, kc, p) at  (((row / 128) * KC + kc) * 128 + row % 128) * 4 + (p ^ ((row >> 2) & 3))
// where piece p holds k = 32 kc + 8 p .. + 7 as fp16.  ds_read_b128 of a fragment (lane = row % 32, piece fixed)
// then touches 16 distinct 16-byte bank groups per 16-lane service group (MI355X_MICROARCH.md, LDS table).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsh_batch.hip.h"

namespace tsh {

constexpr int F16_KC = 32;        // k per chunk
constexpr int F16_GROUP = 128;    // rows per plane block
constexpr int F16_BLOCK_PIECES = F16_GROUP * 4;  // 16-byte pieces per (group, chunk) block = 8 KB

__host__ __device__ __forceinline__ int64_t plane32_piece(int64_t row, int kc, int p, int kchunks) {
  return (((row / F16_GROUP) * kchunks + kc) * F16_GROUP + row % F16_GROUP) * 4 + (p ^ (int)((row >> 2) & 3));
}

struct Half32Args {
  const float *rows;      // n x ld f32
  const float *inv_norm;  // nullable: multiply each row by its 1/|row| first (cosine corpus)
  u32x4 *out;             // plane32 layout
  int64_t ld;
  int64_t first, n;
  int32_t dim, kchunks;   // kchunks = ceil(dim / 32)
  float scale;            // power of two
  const uint32_t *ids;    // nullable: a GATHERED copy -- plane row first + i holds row ids[i] of `rows` (the hub rows)
};

// one thread = 8 consecutive k of one row = one 16-byte piece
static __global__ void __launch_bounds__(256) half_rows32_kernel(Half32Args a) {
  const int64_t per_row = (int64_t)a.kchunks * 4;
  const int64_t total = a.n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = a.first + i / per_row;
    const int pp = (int)(i % per_row), kc = pp >> 2, p = pp & 3;
    const int k0 = kc * 32 + p * 8;
    const int64_t srow = a.ids ? (int64_t)a.ids[i / per_row] : row;
    const float *src = a.rows + srow * a.ld + k0;
    const float mul = a.inv_norm ? a.inv_norm[srow] * a.scale : a.scale;
    f16x8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (_Float16)(k0 + e < a.dim ? src[e] * mul : 0.f);  // round to nearest even
    a.out[plane32_piece(row, kc, p, a.kchunks)] = __builtin_bit_cast(u32x4, h);
  }
}

// ---- the norm-grouped plane (round 6) ---------------------------------------------------------------------------------
// Under L2 / inner product with varying norms a query's survivors are not spread over the corpus: the SHORT rows (L2;
// the long ones under inner product) are near every query, a few thousand rows take most of the ~480 survivors of each
// of a call's 1024 queries, and in the key kernel's epilogue a lane (= one corpus row) that holds more than two
// survivors sends its whole wave tile through the register-by-register walk.  With those rows scattered over the
// corpus a quarter of all wave tiles hold one (the L2 key passes ran 11-14 % behind cosine's, same MFMA work); put
// side by side they fill one wave tile in a hundred.  So the fp16 plane of an L2 / inner-product shard holds its rows
// in another order than the row store: inside every block of PG_ROWS consecutive rows, by norm.  A block maps onto
// itself -- any window of whole blocks (the sample window, a mask's window) holds the same rows in either order, so
// the sample stays an unbiased one and the masks' kept-row counts stay what they were -- and nothing downstream of a
// candidate's row id changes: perm[position] = row travels with the plane, the key kernel reads norms by position
// (psq) and live / mask bits and candidate ids through perm (BatchArgs::row_ids).  The sorted order is ROTATED by a
// block-dependent number of 256-row tiles: with every block's hottest tile at the same offset the persistent key
// kernel's workgroup b (tiles b, b + G, ...; G = 256) would meet either all of them or none (measured on a pre-sorted
// corpus: 8 of 256 workgroups held every crowded tile, 2.2 ms instead of 1.5).  Rows of norm zero (absent /
// quarantined: never live) go last.  The tail behind the last whole block keeps the row order.
constexpr int PG_ROWS = 8192;
struct PlaneGroupArgs {
  const float *sqnorm;    // |v|^2 per row
  uint32_t *perm;         // out, per plane position: the row it holds
  float *psq;             // out, per plane position: that row's |v|^2
  int64_t first;          // first position to (re)write: a multiple of PG_ROWS
  int64_t rows;           // the shard's rows: positions [first, rows) are written
  int32_t longest_first;  // inner product: the longest rows lead a block (L2: the shortest)
};
// one workgroup per block; ranks by counting (a row's rank = the rows of its block in front of it by (norm, place)): 67 M
// compares per block, all blocks side by side -- about a millisecond, once per (re)build of a block
static __global__ void __launch_bounds__(1024) plane_group_kernel(PlaneGroupArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_key[PG_ROWS];
  constexpr int PER = PG_ROWS / 1024;
  const int tid = threadIdx.x;
  const int64_t b0 = a.first + (int64_t)blockIdx.x * PG_ROWS;
  if (b0 + PG_ROWS > a.rows) {  // the tail: row order
    for (int64_t p = b0 + tid; p < a.rows; p += 1024) {
      a.perm[p] = (uint32_t)p;
      a.psq[p] = a.sqnorm[p];
    }
    return;
  }
  // the order key: the norm's leading 19 bits (sign, exponent, 10 of the mantissa: grouping needs no more) above the row's
  // place in the block -- distinct per row, so the ranks are a permutation, and one 32-bit compare per pair
  static_assert(PG_ROWS == 8192, "13 bits of the order key are the row's place in its block");
  for (int i = tid; i < PG_ROWS; i += 1024) {
    const uint32_t u = __float_as_uint(a.sqnorm[b0 + i]);  // (a sum of squares: no sign bit, the bit patterns order like the values)
    const uint32_t kk = (u == 0u || u >= 0x7F800000u) ? 0xFFFFFFFFu : (a.longest_first ? 0x7F800000u - u : u);
    s_key[i] = (kk & 0xFFFFE000u) | (uint32_t)i;
  }
  __syncthreads();
  uint32_t own[PER], rank[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    own[u] = s_key[tid + 1024 * u];
    rank[u] = 0;
  }
  for (int j = 0; j < PG_ROWS; j += 4) {
    const u32x4 k4 = *reinterpret_cast<const u32x4 *>(&s_key[j]);  // (wave-uniform address: one broadcast read)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int u = 0; u < PER; ++u) rank[u] += k4[e] < own[u] ? 1u : 0u;
    }
  }
  const uint32_t rot = 256u * (uint32_t)(((b0 / PG_ROWS) >> 1) & (PG_ROWS / 256 - 1));
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int64_t row = b0 + tid + 1024 * u, pos = b0 + (int64_t)((rank[u] + rot) & (uint32_t)(PG_ROWS - 1));
    a.perm[pos] = (uint32_t)row;
    a.psq[pos] = a.sqnorm[row];
  }
}

// out[i] = src[ids[i]] (the norms of a gathered copy's rows, by position)
static __global__ void __launch_bounds__(256) gather_f32_kernel(const float *src, const uint32_t *ids, float *out, int32_t n) {
  const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (i < n) out[i] = src[ids[i]];
}

// one wave's 64 x 16 B from global (per-lane address) into LDS at lds_dst + 16 * lane (wave-uniform base in M0).
// Invisible to the compiler's s_waitcnt bookkeeping: completion is counted by hand (f16_wait_dma).
__device__ __forceinline__ void f16_dma16(const void *gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}
// the same with a wave-uniform base in an SGPR pair and one per-lane byte offset shared by all pieces of the wave
__device__ __forceinline__ void f16_dma16_s(const void *sbase_any, uint32_t voff, uint32_t lds_dst) {
  // (the base is wave-uniform by construction; where the compiler has lost track of that it holds it in VGPRs, and the
  // "s" constraint fails to assemble: readfirstlane is free when the value already sits in SGPRs)
  const uint64_t pb = (uint64_t)sbase_any;
  const void *sbase = reinterpret_cast<const void *>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(pb >> 32)) << 32) |
                                                     (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)pb));
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}
template <int N>
__device__ __forceinline__ void f16_wait_dma() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

constexpr int F16_HITS = 128;  // per-wave survivor list of one tile (two per lane); fuller tiles take the slow walk

}  // namespace tsh
