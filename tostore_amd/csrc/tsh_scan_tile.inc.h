// tsh_scan_tile.inc.h -- the tile scan's skeleton, written once and included as TEXT into the bodies of scan_kernel,
// scan_f16_kernel and scan_i8_kernel (tsh_kernels.hip.h).  Text, not functions: the register budget of these kernels
// is tuned per width to the last VGPR, and every function boundary tried -- helpers per piece, or the whole unchanged
// body moved into one forced-inline function -- changed register allocation somewhere (more VGPRs, a lower occupancy or
// scratch in some two dozen instantiations; profiles/scan_tile_refactor_isa.txt).  Included as text the three kernels
// compile to exactly what their hand-written copies did.
//
// The including kernel has `ScanArgsQ aq` and, as types / compile-time constants in scope:
//   Store   the row store it reads: RowsF32<METRIC, NT>, RowsF16 or RowsI8 (tsh_kernels.hip.h)
//   NCH, FULL, MASKED, R     chunks per row, d4 == NCH*64, tiles behind live & mask words, rows per register buffer
// and includes this file twice:
//   #define TSH_SCAN_TILE_SETUP   once, at the top of its body: the lane setup.  Leaves a, lane, wave, wpb, stride, has(),
//                                 q[] ... in scope
//   #define TSH_SCAN_TILE_SUM     inside its loop over tiles `t`: the tile's word and the pipelined sum of its rows.
//                                 Leaves `float val` (lane l: the sum, in Store::SUM, of row = t*64+l), `bool alive` (that
//                                 row is scanned) and `uint64_t bits` in scope; a dead tile has stored its gmin and
//                                 `continue`d.  The kernel's own epilogue follows: sum -> stored key(s) and the tile's gmin.
// (no include guard: that is the point)

#if defined(TSH_SCAN_TILE_SETUP)
#undef TSH_SCAN_TILE_SETUP
  static_assert(R == 2 || R == 4 || R == 8, "whole groups of R rows per 8-row batch");
  // one group per batch (R == 8): the buffers alternate between BATCHES, which the loop takes in pairs; a masked tile's
  // batch count may be odd, so a masked scan with R == 8 needs a tail of its own there
  static_assert(R < 8 || !MASKED, "masked tiles with one group per batch are not written yet");
  const ScanArgs &a = aq.a;
  const float *qsrc = scan_query_ptr(a.query);
  constexpr int G = 8 / R;  // groups per batch
  const typename Store::elem *rows = Store::rows(a.rows, a.rows16);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // WAVES bounds the workgroup size; small shards are launched with one wave
  // per workgroup so the dispatcher can balance tiles across CUs
  const int wpb = __builtin_amdgcn_readfirstlane((int)blockDim.x >> 6);
  const int stride = gridDim.x * wpb;
  // All offsets are in ELEMENTS (four per lane and chunk, 256 per chunk), so they are the same for every row store.
  // !FULL: the row ends inside chunk d4/64 and every later chunk is empty (NCH comes from a short list of
  // widths, so more than the last chunk can lie beyond the row).  vmask bit c = this lane's four elements of chunk
  // c exist; lanes without them reload the row's first four (valid memory) and contribute zeros.
  uint32_t vmask = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) vmask |= (FULL || c * 64 + lane < a.d4) ? (1u << c) : 0u;
  auto has = [&](int c) { return FULL || ((vmask >> c) & 1u) != 0u; };
  // (row and query pointers already include + 4 * lane: lanes without data fall back to element 0 of the row --
  // 4 * lane elements further on may be past the end of the last row's allocation when rows are narrow)
  auto off = [&](int c) { return has(c) ? c * 256 : -4 * lane; };
  uint32_t loff[NCH];  // !FULL: this lane's element offset into a row, per chunk (lanes past the row's end: its start)
#pragma unroll
  for (int c = 0; c < NCH; ++c) loff[c] = has(c) ? (uint32_t)(4 * lane + c * 256) : 0u;

  f32x4 q[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    q[c] = *reinterpret_cast<const f32x4 *>(qsrc + 4 * lane + off(c));
    if (!has(c)) q[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (a.query_out && blockIdx.x == 0 && wave == 0) {  // for the rerank kernel
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (has(c))
        *reinterpret_cast<f32x4 *>(a.query_out + 4 * lane + c * 256) = q[c];
  }
  // The kernel's loop over tiles follows:
  //   for (int t = MASKED ? wave * (int)gridDim.x + (int)blockIdx.x : (int)blockIdx.x * wpb + wave; t < a.n_tiles; t += stride)
  // masked scans hand consecutive tiles to different WORKGROUPS: a contiguous id-range
  // filter leaves one run of live tiles, which would otherwise land on a few CUs

#elif defined(TSH_SCAN_TILE_SUM)
#undef TSH_SCAN_TILE_SUM
    const typename Store::elem *tbase = rows + (int64_t)t * 64 * a.ld + 4 * lane;
    // the tile's word: bit r = row t*64+r is scanned (MASKED: live & the caller's mask, made wave-uniform)
    uint64_t bits = ~0ull;
    int cnt = 64;
    if (MASKED) {
      uint64_t w = a.live[t];
      if (a.mask) w &= a.mask[t];
      uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)w);
      uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(w >> 32));
      bits = ((uint64_t)hi << 32) | lo;
      cnt = __popcll(bits);
      if (cnt == 0) {
        if (lane == 0) {
          a.gmin[t] = KEY_DEAD;  // keys[] of a dead tile stay stale: every reader checks gmin first
          if constexpr (Store::LOWER_MIN) a.gmin[a.n_tiles + t] = KEY_DEAD;  // (the coarse scan's second minimum)
        }
        continue;
      }
    }
    const int nb = MASKED ? (cnt + 7) >> 3 : 8;  // 8-row batches, wave-uniform

    // two register buffers of R rows; they hold what was loaded, widened only where it is consumed, behind the fence,
    // so a load never waits for its own conversion
    typename Store::chunk v[2][R][NCH];
    uint64_t rem = bits;
    int last = 0, next_dense = 0;
    auto load_group = [&](int buf) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        int r;
        if (MASKED) {  // next live row (a short last batch repeats the final row)
          if (rem) {
            last = __builtin_ctzll(rem);
            rem &= rem - 1;
          }
          r = last;
        } else {
          r = next_dense++;
        }
        if (FULL) {
          const typename Store::elem *rp = tbase + (int64_t)r * a.ld;
#pragma unroll
          for (int c = 0; c < NCH; ++c) v[buf][j][c] = Store::load(rp + off(c));
        } else {
          // a lane's offset differs from chunk to chunk here (lanes past the row's end fall back to its start), which as
          // a 64-bit address per row and chunk cost R x NCH register pairs and spilled (f32, d = 384: 30 registers, d = 1000:
          // 164; 0.62 / 0.42 of the HBM peak where full widths reach 0.82): the row's start is wave-uniform -- a scalar
          // base -- and the lane's part a 32-bit offset per chunk, computed once
          // (through readfirstlane: otherwise the optimiser derives the next row's addresses from this row's, per lane)
          const uint64_t rbi = (uint64_t)(rows + ((int64_t)t * 64 + r) * a.ld);
          const typename Store::elem *rb = reinterpret_cast<const typename Store::elem *>(
              ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(rbi >> 32)) << 32) |
              (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)rbi));
#pragma unroll
          for (int c = 0; c < NCH; ++c) v[buf][j][c] = Store::load(rb + loff[c]);
        }
      }
    };

    float val = 0.f;
    // The previous tile's key / gmin stores share vmcnt with the loads, and stores may retire out of order with
    // loads: while one MIGHT be pending the compiler must wait for vmcnt(0) instead of counting.  Retire them here.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    load_group(0);
    // One 8-row batch, its first group in buffer BUF.  Per group: the other buffer's loads go out first, then this one's
    // chunks are widened and consumed.  The LAST batch is a separate instance without the trailing load instead of an
    // `if` inside the loop: behind a branch the compiler's s_waitcnt insertion no longer knows which loads are in flight
    // and waits for vmcnt(0) -- the group just issued included -- before every group's arithmetic.
    auto batch = [&](int b, auto BUF, auto LAST) {
      constexpr int buf0 = decltype(BUF)::value;
      float acc[8];
#pragma unroll
      for (int k = 0; k < G; ++k) {
        if (!(decltype(LAST)::value && k == G - 1)) load_group((buf0 + k + 1) & 1);
        TSH_FENCE();
#pragma unroll
        for (int j = 0; j < R; ++j) {
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < NCH; ++c)  // (!FULL: lanes past the row's end sit the chunk out)
            if (has(c)) s = accum4<Store::SUM>(s, q[c], Store::widen(v[(buf0 + k) & 1][j][c]));
          // tie the finished sum to the fence: pure math would otherwise be
          // sunk below the next group's loads, keeping every buffer live
          asm volatile("" : "+v"(s)::"memory");
          acc[k * R + j] = s;
        }
        TSH_FENCE();
      }
      // octet partial of row (lane&7) of this batch, then across the 8 octets
      float o = treduce8<0>(acc, lane);
      o += __shfl_xor(o, 8);
      o += __shfl_xor(o, 16);
      o += __shfl_xor(o, 32);
      if ((lane >> 3) == b) val = o;  // slot b*8 + (lane&7) == lane
    };
    if constexpr (G > 1) {
#pragma nounroll
      for (int b = 0; b < nb - 1; ++b) batch(b, std::integral_constant<int, 0>{}, std::false_type{});
      batch(nb - 1, std::integral_constant<int, 0>{}, std::true_type{});
    } else {
#pragma nounroll
      for (int b = 0; b < nb - 2; b += 2) {
        batch(b, std::integral_constant<int, 0>{}, std::false_type{});
        batch(b + 1, std::integral_constant<int, 1>{}, std::false_type{});
      }
      batch(nb - 2, std::integral_constant<int, 0>{}, std::false_type{});
      batch(nb - 1, std::integral_constant<int, 1>{}, std::true_type{});
    }
    // dense: val = the sum of row t*64+lane; masked: of the lane-th live row

    const int64_t row = (int64_t)t * 64 + lane;
    bool alive;
    if (MASKED) {
      // expand compact slots back to row positions
      uint64_t below = bits & ((1ull << lane) - 1ull);
      int rank = __popcll(below);
      val = __shfl(val, rank);
      alive = (bits >> lane) & 1ull;
    } else {
      alive = row < a.n;
    }

#else
#error "define TSH_SCAN_TILE_SETUP or TSH_SCAN_TILE_SUM before including tsh_scan_tile.inc.h"
#endif
