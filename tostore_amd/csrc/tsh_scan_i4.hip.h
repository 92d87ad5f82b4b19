// tsh_scan_i4.hip.h -- a 4-bit first pass in front of the coarse int8 scan of an L2 shard (gfx950, wave = 64).
//   A  scan_i4_kernel   dense, L2.  Reads the 4-bit plane: the high nibbles of the int8 copy's biased bytes, half a byte per
//                       element, and per row the int8 copy's scale and rho = |v - recon4|_2.  Stores per row the LOWER side
//                       of its key's band (tsh_scan_i4_band.h) and per tile the minimum of the UPPER sides -- into buffers of
//                       its own, so that B's keys and minima do not alias them.
//   T  i4_tau_kernel    one workgroup: tau = the k-th smallest upper minimum (select_tau).  k distinct tiles hold a row whose
//                       exact key is <= tau, so every row of the top k -- and every row tied with the k-th -- has a lower side
//                       <= tau.  Fewer than k live tiles: tau = KEY_NAN, every row survives.
//   W  i4_mask_kernel   a wave per tile: the ballot of lower sides <= tau is the tile's word of an ordinary row mask; the
//                       survivors' total (i4_total_kernel, one workgroup beside the tail) reaches the host in pinned memory.
//   B  scan_i8_kernel<MASKED> behind W's words, then the int8 route's tail (tsh_scan_i8.hip.h), both unchanged.
//
// The plane.  A tile of 64 rows is groups x 64 x 16 bytes: [group][row][16 B], a group = 32 consecutive elements of a row
// (SCAN_I4_GROUP; a row of ld elements has ceil(ld / 32) groups -- ld / 2 bytes per row where ld is a multiple of 32, the
// last group padded with the code of zero otherwise).  Dword w of a group holds elements 8 w .. 8 w + 7: byte b its
// elements 8 w + b (low nibble) and 8 w + 4 + b (high nibble), so two masks leave eight codes where v_cvt_f32_ubyteN
// takes them.  In A a LANE owns a ROW: a wave's 16-byte loads are 1 KiB of consecutive memory, the query's elements are
// the same for all lanes -- scalar loads, an SGPR operand of each FMA -- and a row's sum never crosses lanes.
#pragma once

#include "tsh_kernels.hip.h"
#include "tsh_scan_i4_band.h"

namespace tsh {

typedef uint32_t u32x4_i4 __attribute__((ext_vector_type(4)));

struct ScanI4Args {
  const u32x4_i4 *plane;  // n_tiles x groups x 64 x 16 B
  const float *query;     // ld floats; NULL: the query rides in the kernel-argument segment (ScanI4ArgsQ::q)
  const float *scale8;    // the int8 copy's per-row scales
  const float *rho;       // |v_i - recon4_i|_2, rounded up
  const float *sqnorm;    // |v_i|^2
  uint32_t *keys;         // n_tiles * 64 lower sides
  uint32_t *gmin;         // n_tiles minima of upper sides
  int64_t n;              // rows
  int32_t n_tiles, ld, groups, pad_;
  float qbias, a_s, a_r, a_c, a_v, beta;  // ScanI4Band
};
struct ScanI4ArgsQ {
  ScanI4Args a;
  float q[SCAN_Q_INLINE];
};
static_assert(sizeof(ScanI4ArgsQ) <= 4096, "kernel arguments are limited to 4 KiB");

typedef const float __attribute__((address_space(4))) * i4_q_ptr;  // constant address space: scalar loads

// byte N of a word as a float, one instruction each.  Written out: left to itself the compiler undoes the two masks below
// and extracts every nibble with a shift and a mask of its own, half as many instructions again
#define TSH_I4_UBYTE(N)                                                       \
  __device__ __forceinline__ float i4_ubyte##N(uint32_t x) {                  \
    float f;                                                                  \
    asm("v_cvt_f32_ubyte" #N " %0, %1" : "=v"(f) : "v"(x));                   \
    return f;                                                                 \
  }
TSH_I4_UBYTE(0) TSH_I4_UBYTE(1) TSH_I4_UBYTE(2) TSH_I4_UBYTE(3)
#undef TSH_I4_UBYTE

// four codes -- the bytes of m, a dword of a group masked to its low or its high nibbles -- against four query elements:
// one FMA on each of the four chains
__device__ __forceinline__ void scan_i4_quad(uint32_t m, const float (&q)[4], float (&acc)[SCAN_I4_ACC]) {
  acc[0] = __builtin_fmaf(i4_ubyte0(m), q[0], acc[0]);
  acc[1] = __builtin_fmaf(i4_ubyte1(m), q[1], acc[1]);
  acc[2] = __builtin_fmaf(i4_ubyte2(m), q[2], acc[2]);
  acc[3] = __builtin_fmaf(i4_ubyte3(m), q[3], acc[3]);
}
// one group of a row: 32 codes against the 32 query elements at qg, eight FMAs on each chain.  quads: how many of the
// group's eight quads of elements the row has (wave-uniform; 8 but for a row that ends inside its last group)
template <bool WHOLE>
__device__ __forceinline__ void scan_i4_group(u32x4_i4 x, i4_q_ptr qg, int quads, float (&acc)[SCAN_I4_ACC]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (WHOLE || i < quads) {
      const uint32_t m = (i & 1) ? (x[i >> 1] >> 4) & 0x0F0F0F0Fu : x[i >> 1] & 0x0F0F0F0Fu;
      const float q[4] = {qg[4 * i], qg[4 * i + 1], qg[4 * i + 2], qg[4 * i + 3]};
      scan_i4_quad(m, q, acc);
    }
  }
}

// the band of one row (the probe forms it with the same arithmetic)
__device__ __forceinline__ float scan_i4_w(const ScanI4Args &a, float sc, float rho, float sq) {
  const float wq = fminf(a.a_s * sc, __builtin_fmaf(a.a_r, rho, a.a_c * sc));
  return wq + __builtin_fmaf(a.a_v, __builtin_sqrtf(sq), a.beta);
}

// A.  One tile per wave and trip; U groups per register buffer, two buffers: the next U loads are out while these U are
// consumed.  Loads past the row's last full group are clamped to it (in bounds) and not consumed.
template <int U>
__global__ void __launch_bounds__(256) scan_i4_kernel(ScanI4ArgsQ aq) {
  const ScanI4Args &a = aq.a;
  typedef const char __attribute__((address_space(4))) * karg_ptr;
  const i4_q_ptr qsrc = a.query ? (i4_q_ptr)(uint64_t)a.query
                                : (i4_q_ptr)((karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(ScanI4ArgsQ, q));
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ngf = a.ld >> 5, tail = a.ld & 31;  // full groups; elements of the last, partial one
  const int last = a.groups - 1;
  for (int t = (int)blockIdx.x * 4 + wave; t < a.n_tiles; t += (int)gridDim.x * 4) {
    const u32x4_i4 *p = a.plane + (int64_t)t * a.groups * 64 + lane;
    float acc[SCAN_I4_ACC] = {0.f, 0.f, 0.f, 0.f};
    u32x4_i4 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = __builtin_nontemporal_load(p + (int64_t)(u < last ? u : last) * 64);
    for (int g = 0; g < ngf; g += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int gn = g + U + u;
        nxt[u] = __builtin_nontemporal_load(p + (int64_t)(gn < last ? gn : last) * 64);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (g + u < ngf) scan_i4_group<true>(cur[u], qsrc + (g + u) * 32, 8, acc);  // (wave-uniform)
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    // the row ends inside its last group: only the quads it has (the rest are the code of zero, and no query element)
    if (tail) scan_i4_group<false>(__builtin_nontemporal_load(p + (int64_t)ngf * 64), qsrc + ngf * 32, tail >> 2, acc);
    const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const int64_t row = (int64_t)t * 64 + lane;
    const bool alive = row < a.n;
    const float sc = alive ? a.scale8[row] : 0.f;
    const float rho = alive ? a.rho[row] : 0.f;
    const float sq = alive ? a.sqnorm[row] : 0.f;
    const float dot = sc * __builtin_fmaf(16.f, sum, -a.qbias);
    const float x = __builtin_fmaf(-2.f, dot, sq);
    const float w = scan_i4_w(a, sc, rho, sq);
    const uint32_t lower = alive ? f2key(x - w) : KEY_DEAD;
    a.keys[row] = lower;
    const uint32_t m = wave_min_u32(alive ? f2key(x + w) : KEY_DEAD);
    if (lane == 0) a.gmin[t] = m;
  }
}

// every row's band (tsh_probe_scan_i4_keys): what scan_i4_kernel took off / added to its key
static __global__ void __launch_bounds__(256) scan_i4_w_kernel(ScanI4Args a, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.n) out[i] = scan_i4_w(a, a.scale8[i], a.rho[i], a.sqnorm[i]);
}

// T.  ctl[0] = tau
template <bool IN_REGS>
__global__ void __launch_bounds__(SEL_THREADS) i4_tau_kernel(const uint32_t *gmin, int32_t n_tiles, int32_t k, uint32_t *__restrict__ ctl) {
  __shared__ SelectTauLds<SEL_THREADS> s_t;
  uint32_t g[SEL_VPT];
  select_tau<SEL_THREADS, IN_REGS>(gmin, n_tiles, (uint32_t)k, false, g, s_t);
  if (threadIdx.x == 0) ctl[0] = s_t.tau;  // (<= KEY_NAN < KEY_DEAD: no absent row survives)
}

// W.  mask[t] bit r = row 64 t + r survives A.  Nothing but loads, a ballot and a store: no counter is shared between
// workgroups (device-wide atomics and fences in every workgroup cost a hundred microseconds beside a streaming scan)
static __global__ void __launch_bounds__(256) i4_mask_kernel(const uint32_t *keys, int32_t n_tiles, uint64_t *__restrict__ mask,
                                                             const uint32_t *ctl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = (int)blockIdx.x * 4 + wave;
  if (t >= n_tiles) return;
  const uint64_t b = __ballot(keys[(int64_t)t * 64 + lane] <= ctl[0]);
  if (lane == 0) mask[t] = b;
}

// The survivors' total, for the host's deny rule: one workgroup adds up the popcounts of W's words and leaves the sum in
// pinned host memory.  Runs with the tail, off the scan streams.
static __global__ void __launch_bounds__(1024) i4_total_kernel(const uint64_t *mask, int32_t n_tiles, uint32_t *host_total) {
  __shared__ uint32_t s_sum[16];
  uint32_t c = 0;
  for (int t = threadIdx.x; t < n_tiles; t += 1024) c += (uint32_t)__popcll(mask[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) total += s_sum[i];
    *host_total = total;
  }
}

// rows [r0, r1) of the int8 copy -> the 4-bit plane and rho: a wave per row, a lane per dword of eight codes.  rho is
// summed in f64 against the f32 rows (s_i times an integer is exact there), over the row's dim elements -- the pad elements
// up to ld meet no query element -- and rounded up.  Elements past dim: the code of zero (biased byte 128).
static __global__ void __launch_bounds__(256) rows4_convert_kernel(const float *rows, const uint8_t *rows8, const float *scale8,
                                                                   uint32_t *plane, float *rho, int64_t ld, int dim, int groups,
                                                                   int64_t r0, int64_t r1) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  for (int64_t r = r0 + w0; r < r1; r += nw) {
    const double s = (double)scale8[r];
    const float *src = rows + r * ld;
    const uint8_t *src8 = rows8 + r * ld;
    uint32_t *dst = plane + ((r >> 6) * groups * 64 + (r & 63)) * 4;
    double ss = 0.0;
    for (int i = lane; i < groups * 4; i += 64) {  // dword i & 3 of group i >> 2: elements 8 i .. 8 i + 7
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t j = (int64_t)8 * i + e;
        uint32_t h = 8u;
        if (j < ld) {
          h = (uint32_t)src8[j] >> 4;
          if (j < dim) {
            const double diff = (double)src[j] - s * (double)(16 * (int)h + 8 - 128);
            ss += diff * diff;
          }
        }
        word |= h << (8 * (e & 3) + 4 * (e >> 2));
      }
      dst[(int64_t)(i >> 2) * 256 + (i & 3)] = word;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const double x = __builtin_sqrt(ss) * (1.0 + 1e-6);
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);  // (positive and finite: the next float up)
    if (lane == 0) rho[r] = f;
  }
}

}  // namespace tsh
