// pp_lovasz.hip -- libpacingpseudo_lov.so (include/pacingpseudo_lov.h): a segmented, stable, descending radix sort on the device and
// the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) built on it.  S segments of n slots each lie back to back; a segment is
// cut into tiles of PLOV_TILE slots, one block per (segment, tile), so one launch sequence serves every segment whatever S and n are.
//   * lov_hist_kernel      the tile's histogram of one 8-bit digit into table[segment][digit][tile];
//   * lov_scan_kernel      exclusive scan of every segment's digit-major table in place, one block per segment, or for a long table
//                          per chunk with the chunks' sums scanned in between (also the scan of the tiles' foreground counts: the
//                          second, small pass that carries the scan of fg across blocks);
//   * lov_scatter_kernel   a wave takes 64 consecutive keys per round, ranks equal digits among them by eight ballots (match), keeps
//                          the digit's running count of the wave in LDS; the waves' counts are stacked in wave order on the scanned
//                          table entry.  Equal digits keep their order: least-significant digit first, four passes, the sort is stable;
//   * lov_key_kernel       the soft-max once per pixel, K keys and payloads (slot in the segment | fg bit | ignored bit);
//   * lov_fgcount_kernel / lov_weight_kernel   the segmented inclusive scan of fg along the sorted order, the increments g_i from the
//                          integer counts in double, the tile's sum of e_i g_i in double, g scattered back to pixel order;
//   * lov_segsum_kernel / lov_final_kernel     fixed-order sums: tiles -> segment -> image -> loss; which segments are averaged and
//                          the scale of each is decided here, on the device;
//   * lov_bwd_kernel       sign, scale, upstream gradient and the soft-max Jacobian in one pass over the pixels.
// Keys are stored INVERTED and sorted ascending, which is the descending order with ties in ascending slot order.  A digit is
// (key >> shift) & 255: any bit pattern of a key stays inside its histogram.  No floating-point atomics anywhere.
// Self-contained on purpose: the per-step library's symbol list is fixed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "pacingpseudo_lov.h"

#define PLOV_VERSION 100
#define PLOV_THREADS 256
#define PLOV_WAVES (PLOV_THREADS / 64)
#define PLOV_ITEMS 8
#define PLOV_TILE (PLOV_THREADS * PLOV_ITEMS)
#define PLOV_RADIX 256
#define PLOV_PASSES 4
#define PLOV_SCAN_CHUNK 4096      // words per block of a long scan
#define PLOV_SCAN_SHORT 8192      // up to this many words per segment: one block per segment
#define PLOV_MIN_K 2
#define PLOV_MAX_K 32
#define PLOV_FG 0x80000000u
#define PLOV_IGN 0x40000000u
#define PLOV_POS 0x3FFFFFFFu

static thread_local char g_lov_err[512] = "";

static void lov_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_lov_err, sizeof(g_lov_err), fmt, ap);
  va_end(ap);
}

#define LOV_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      lov_set_error(__VA_ARGS__);  \
      return -1;                   \
    }                              \
  } while (0)

static int lov_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    lov_set_error("%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- block helpers
// exclusive prefix of v over the block's threads, the block's total in *total; sh: PLOV_WAVES words of LDS, free again on return
__device__ __forceinline__ unsigned lov_block_scan(unsigned v, unsigned* total, unsigned* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  unsigned woff = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < PLOV_WAVES; ++i) {
    const unsigned s = sh[i];
    if (i < w) woff += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return woff + inc - v;
}

// the block's sum of v in a fixed order (xor tree in the wave, then the waves left to right); valid in thread 0
__device__ __forceinline__ double lov_block_sum_d(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int i = 1; i < PLOV_WAVES; ++i) r += sh[i];
  return r;
}

// ---------------------------------------------------------------------------------------------------------------- the sort
__global__ __launch_bounds__(PLOV_THREADS) void lov_hist_kernel(const unsigned* __restrict__ keys, unsigned n, unsigned T, int shift,
                                                                unsigned* __restrict__ table) {
  __shared__ unsigned hist[PLOV_RADIX];
  const unsigned seg = blockIdx.x / T, tile = blockIdx.x - seg * T;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* __restrict__ k = keys + (size_t)seg * n;
  const unsigned first = tile * PLOV_TILE + threadIdx.x;
#pragma unroll
  for (int r = 0; r < PLOV_ITEMS; ++r) {
    const unsigned idx = first + r * PLOV_THREADS;
    if (idx < n) atomicAdd(&hist[(k[idx] >> shift) & (PLOV_RADIX - 1)], 1u);
  }
  __syncthreads();
  table[((size_t)seg * PLOV_RADIX + threadIdx.x) * T + tile] = hist[threadIdx.x];
}

// exclusive scan in place of `len` words per segment, cut into C chunks of `chunk` words, one block per (segment, chunk), 4 words per
// thread and round.  carries (may be null: 0) holds what lies in front of each chunk in its segment; totals (may be null) receives
// carry + the chunk's sum.  A short segment is one chunk; a long one takes three launches: lov_chunk_sum_kernel, this kernel over the
// chunks' sums (one chunk per segment), this kernel over the chunks with those carries -- no block waits for another.
__global__ __launch_bounds__(PLOV_THREADS) void lov_scan_kernel(unsigned* __restrict__ table, size_t len, size_t chunk, unsigned C,
                                                                const unsigned* __restrict__ carries, unsigned* __restrict__ totals) {
  __shared__ unsigned sh[PLOV_WAVES];
  const unsigned seg = blockIdx.x / C, c = blockIdx.x - seg * C;
  unsigned* __restrict__ p = table + (size_t)seg * len;
  const size_t lo = (size_t)c * chunk, hi = lo + chunk < len ? lo + chunk : len;
  unsigned carry = carries != nullptr ? carries[blockIdx.x] : 0u;
  for (size_t base = lo; base < hi; base += 4 * PLOV_THREADS) {
    const size_t i0 = base + 4 * (size_t)threadIdx.x;
    unsigned v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = i0 + j < hi ? p[i0 + j] : 0u;
      s += v[j];
    }
    unsigned tot;
    unsigned run = carry + lov_block_scan(s, &tot, sh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < hi) p[i0 + j] = run;
      run += v[j];
    }
    carry += tot;
  }
  if (totals != nullptr && threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(PLOV_THREADS) void lov_chunk_sum_kernel(const unsigned* __restrict__ table, size_t len, size_t chunk, unsigned C,
                                                                     unsigned* __restrict__ sums) {
  __shared__ unsigned sh[PLOV_WAVES];
  const unsigned seg = blockIdx.x / C, c = blockIdx.x - seg * C;
  const unsigned* __restrict__ p = table + (size_t)seg * len;
  const size_t lo = (size_t)c * chunk, hi = lo + chunk < len ? lo + chunk : len;
  unsigned s = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += PLOV_THREADS) s += p[i];
  unsigned tot;
  lov_block_scan(s, &tot, sh);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PLOV_THREADS) void lov_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ pin,
                                                                   unsigned* __restrict__ kout, unsigned* __restrict__ pout, unsigned n,
                                                                   unsigned T, int shift, const unsigned* __restrict__ table) {
  __shared__ unsigned cnt[PLOV_WAVES][PLOV_RADIX];
  const unsigned seg = blockIdx.x / T, tile = blockIdx.x - seg * T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < PLOV_WAVES; ++i) cnt[i][threadIdx.x] = 0;
  __syncthreads();
  const size_t sb = (size_t)seg * n;
  const unsigned first = tile * PLOV_TILE + (unsigned)w * (64 * PLOV_ITEMS) + (unsigned)lane;
  const unsigned long long below = (1ull << lane) - 1ull;
  volatile unsigned* mine = cnt[w];
  unsigned key[PLOV_ITEMS], pay[PLOV_ITEMS], rank[PLOV_ITEMS];
#pragma unroll
  for (int r = 0; r < PLOV_ITEMS; ++r) {
    const unsigned idx = first + r * 64;
    const bool act = idx < n;
    key[r] = act ? kin[sb + idx] : 0u;
    pay[r] = act ? pin[sb + idx] : 0u;
    const unsigned d = (key[r] >> shift) & (PLOV_RADIX - 1);
    unsigned long long m = __ballot(act);      // the lanes of this round that hold a key with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    const unsigned prev = mine[d];               // equal addresses broadcast; read by all before the first of them writes
    if (act && (m & below) == 0ull) mine[d] = prev + (unsigned)__popcll(m);
    rank[r] = prev + (unsigned)__popcll(m & below);
  }
  __syncthreads();
  {
    unsigned base = table[((size_t)seg * PLOV_RADIX + threadIdx.x) * T + tile];
#pragma unroll
    for (int i = 0; i < PLOV_WAVES; ++i) {
      const unsigned c = cnt[i][threadIdx.x];
      cnt[i][threadIdx.x] = base;
      base += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < PLOV_ITEMS; ++r) {
    const unsigned idx = first + r * 64;
    const unsigned d = (key[r] >> shift) & (PLOV_RADIX - 1);
    const unsigned dst = cnt[w][d] + rank[r];
    if (idx < n && dst < n) {      // dst < n holds by construction; the test keeps a store inside the segment whatever happens
      kout[sb + dst] = key[r];
      pout[sb + dst] = pay[r];
    }
  }
}

// keys of sort_descending: the order-preserving integer image of a float, inverted.  -0 is keyed as +0 and every NaN as the one key
// above +inf (what v + 0.0f and a canonical NaN would give, formed on the bits so that it does not depend on the denormal mode).
__global__ __launch_bounds__(PLOV_THREADS) void lov_float_key_kernel(const float* __restrict__ v, unsigned n, size_t total,
                                                                     unsigned* __restrict__ keys, unsigned* __restrict__ pay) {
  const size_t i = (size_t)blockIdx.x * PLOV_THREADS + threadIdx.x;
  if (i >= total) return;
  unsigned b = __float_as_uint(v[i]);
  const unsigned mag = b & 0x7FFFFFFFu;
  if (mag == 0u) b = 0u;
  unsigned asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if (mag > 0x7F800000u) asc = 0xFFFFFFFFu;
  keys[i] = ~asc;
  pay[i] = (unsigned)(i % n);
}

__global__ __launch_bounds__(PLOV_THREADS) void lov_sort_finish_kernel(const float* __restrict__ v, const unsigned* __restrict__ pay,
                                                                       unsigned n, size_t total, float* __restrict__ sorted,
                                                                       int* __restrict__ perm) {
  const size_t i = (size_t)blockIdx.x * PLOV_THREADS + threadIdx.x;
  if (i >= total) return;
  const unsigned p = pay[i];
  const size_t sb = i - i % n;
  perm[i] = (int)p;
  sorted[i] = p < n ? v[sb + p] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- the loss
struct LovShape {
  int K, HW, per_image, has_ignore;
  long long ignore_index;
  unsigned total;      // N * H * W
};

__device__ __forceinline__ bool lov_valid(long long t, const LovShape& s) {
  return t >= 0 && t < (long long)s.K && !(s.has_ignore && t == s.ignore_index);
}

// soft-max numerators of the pixel at `base` (max-subtracted), their sum returned
template <int MK>
__device__ __forceinline__ float lov_softmax(const float* __restrict__ z, size_t base, int K, int HW, float e[MK]) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    e[k] = k < K ? z[base + (size_t)k * HW] : -INFINITY;
    mx = fmaxf(mx, e[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    e[k] = k < K ? expf(e[k] - mx) : 0.f;
    s += e[k];
  }
  return s;      // fmaxf drops a NaN operand, expf does not: a non-finite logit makes s, and with it every probability of its pixel, NaN
}

template <int MK>
__global__ __launch_bounds__(PLOV_THREADS) void lov_key_kernel(const float* __restrict__ z, const long long* __restrict__ t, LovShape sh,
                                                               unsigned* __restrict__ keys, unsigned* __restrict__ pay,
                                                               float* __restrict__ errors) {
  const unsigned i = blockIdx.x * PLOV_THREADS + threadIdx.x;
  if (i >= sh.total) return;
  const unsigned n = i / (unsigned)sh.HW, px = i - n * (unsigned)sh.HW;
  float e[MK];
  const float s = lov_softmax<MK>(z, (size_t)n * sh.K * sh.HW + px, sh.K, sh.HW, e);
  const long long tv = t[i];
  const bool valid = lov_valid(tv, sh);
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    if (k < sh.K) {
      const bool fg = valid && tv == (long long)k;
      const float err = fabsf((fg ? 1.f : 0.f) - e[k] / s);
      // valid: 1 + the bits of err in [0, 1], inverted; ignored: strictly behind every valid one
      const unsigned key = valid ? ~(__float_as_uint(err) + 1u) : 0xFFFFFFFFu;
      const size_t at = sh.per_image ? ((size_t)n * sh.K + k) * sh.HW + px : (size_t)k * sh.total + i;
      keys[at] = key;
      pay[at] = (sh.per_image ? px : i) | (fg ? PLOV_FG : 0u) | (valid ? 0u : PLOV_IGN);
      if (errors != nullptr) errors[(size_t)k * sh.total + i] = valid ? err : 0.f;
    }
  }
}

__global__ __launch_bounds__(PLOV_THREADS) void lov_fgcount_kernel(const unsigned* __restrict__ pay, unsigned n, unsigned T,
                                                                   unsigned* __restrict__ tilefg) {
  __shared__ unsigned sh[PLOV_WAVES];
  const unsigned seg = blockIdx.x / T, tile = blockIdx.x - seg * T;
  const unsigned* __restrict__ p = pay + (size_t)seg * n;
  const unsigned first = tile * PLOV_TILE + threadIdx.x;
  unsigned c = 0;
#pragma unroll
  for (int r = 0; r < PLOV_ITEMS; ++r) {
    const unsigned idx = first + r * PLOV_THREADS;
    if (idx < n) c += p[idx] >> 31;
  }
  unsigned tot;
  lov_block_scan(c, &tot, sh);
  if (threadIdx.x == 0) tilefg[blockIdx.x] = tot;
}

// tilefg holds the exclusive scan over the segment's tiles, G the segment's foreground count.  A thread takes PLOV_ITEMS consecutive
// slots of the sorted order.  With c_i the running fg count, U_i = G + i - c_i and I_i = G - c_i (integers):
//   g_i = J_i - J_{i-1} = 1 / U_i when fg_i = 1 and I_i / ((U_i - 1) U_i) when fg_i = 0; for G = 0, g_1 = 1 and g_i = 0 after it.
__global__ __launch_bounds__(PLOV_THREADS) void lov_weight_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ pay,
                                                                  unsigned n, unsigned T, const unsigned* __restrict__ tilefg,
                                                                  const unsigned* __restrict__ G, LovShape sh, float* __restrict__ gbuf,
                                                                  int* __restrict__ perm, double* __restrict__ partial) {
  __shared__ unsigned shu[PLOV_WAVES];
  __shared__ double shd[PLOV_WAVES];
  const unsigned seg = blockIdx.x / T, tile = blockIdx.x - seg * T;
  const size_t sb = (size_t)seg * n;
  const unsigned first = tile * PLOV_TILE + threadIdx.x * PLOV_ITEMS;
  unsigned key[PLOV_ITEMS], py[PLOV_ITEMS], mine = 0;
#pragma unroll
  for (int j = 0; j < PLOV_ITEMS; ++j) {
    const unsigned idx = first + j;
    key[j] = idx < n ? keys[sb + idx] : 0xFFFFFFFFu;
    py[j] = idx < n ? pay[sb + idx] : PLOV_IGN;
    mine += py[j] >> 31;
  }
  unsigned tot;
  unsigned c = tilefg[blockIdx.x] + lov_block_scan(mine, &tot, shu);
  const unsigned Gs = G[seg];
  const unsigned img = sh.per_image ? seg / (unsigned)sh.K : 0u, cls = sh.per_image ? seg - img * (unsigned)sh.K : seg;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < PLOV_ITEMS; ++j) {
    const unsigned idx = first + j;
    if (idx < n) {
      const bool fg = (py[j] & PLOV_FG) != 0u, ign = (py[j] & PLOV_IGN) != 0u;
      c += fg ? 1u : 0u;
      double g = 0.0;
      if (!ign) {
        if (Gs == 0u) {
          g = idx == 0u ? 1.0 : 0.0;
        } else {
          const double U = (double)Gs + (double)(idx + 1u) - (double)c;
          g = fg ? 1.0 / U : ((double)Gs - (double)c) / ((U - 1.0) * U);
        }
        acc += (double)__uint_as_float(~key[j] - 1u) * g;
      }
      const unsigned pixel = img * n + (py[j] & PLOV_POS);
      if (pixel < sh.total) gbuf[(size_t)cls * sh.total + pixel] = (float)g;
      if (perm != nullptr) perm[sb + idx] = (int)pixel;
    }
  }
  const double bsum = lov_block_sum_d(acc, shd);
  if (threadIdx.x == 0) partial[blockIdx.x] = bsum;
}

// one wave per segment: its tiles' partial sums, lanes striding over the tiles, then the xor tree
__global__ __launch_bounds__(PLOV_THREADS) void lov_segsum_kernel(const double* __restrict__ partial, unsigned S, unsigned T,
                                                                  double* __restrict__ segloss) {
  const unsigned seg = blockIdx.x * PLOV_WAVES + (threadIdx.x >> 6);
  if (seg >= S) return;
  double a = 0.0;
  for (unsigned t = threadIdx.x & 63; t < T; t += 64) a += partial[(size_t)seg * T + t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((threadIdx.x & 63) == 0) segloss[seg] = a;
}

// one block: per image (the whole batch is the one "image" without per_image) the mean over the averaged segments, then the mean over
// the images.  segscale[seg] = 1 / (averaged segments of the image * images), 0 for a segment that is not averaged.
__global__ __launch_bounds__(PLOV_THREADS) void lov_final_kernel(const double* __restrict__ segloss, const unsigned* __restrict__ G,
                                                                 unsigned nimg, int K, int classes_all, float* __restrict__ segscale,
                                                                 float* __restrict__ loss) {
  __shared__ double shd[PLOV_WAVES];
  double acc = 0.0;
  for (unsigned img = threadIdx.x; img < nimg; img += PLOV_THREADS) {
    unsigned cnt = 0;
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      const size_t seg = (size_t)img * K + k;
      if (classes_all || G[seg] > 0u) {
        ++cnt;
        s += segloss[seg];
      }
    }
    const float sc = cnt ? (float)(1.0 / ((double)cnt * (double)nimg)) : 0.f;
    for (int k = 0; k < K; ++k) {
      const size_t seg = (size_t)img * K + k;
      segscale[seg] = (classes_all || G[seg] > 0u) ? sc : 0.f;
    }
    if (cnt) acc += s / (double)cnt;
  }
  const double tot = lov_block_sum_d(acc, shd);
  if (threadIdx.x == 0) loss[0] = (float)(tot / (double)nimg);
}

template <int MK>
__global__ __launch_bounds__(PLOV_THREADS) void lov_bwd_kernel(const float* __restrict__ z, const long long* __restrict__ t, LovShape sh,
                                                               const float* __restrict__ gbuf, const float* __restrict__ segscale,
                                                               const float* __restrict__ grad, float* __restrict__ dz) {
  const unsigned i = blockIdx.x * PLOV_THREADS + threadIdx.x;
  if (i >= sh.total) return;
  const unsigned n = i / (unsigned)sh.HW, px = i - n * (unsigned)sh.HW;
  const size_t base = (size_t)n * sh.K * sh.HW + px;
  float e[MK], dp[MK];
  const float s = lov_softmax<MK>(z, base, sh.K, sh.HW, e);
  const long long tv = t[i];
  const bool valid = lov_valid(tv, sh);
  const float up = grad[0];
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < MK; ++k) {
    dp[k] = 0.f;
    if (k < sh.K) {
      e[k] = e[k] / s;
      if (valid) {
        const float d = e[k] - (tv == (long long)k ? 1.f : 0.f);
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);      // 0 at 0 (and NaN stays NaN)
        dp[k] = sg * gbuf[(size_t)k * sh.total + i] * (segscale[sh.per_image ? n * (unsigned)sh.K + k : (unsigned)k] * up);
      }
      dot += e[k] * dp[k];
    }
  }
#pragma unroll
  for (int k = 0; k < MK; ++k)
    if (k < sh.K) dz[base + (size_t)k * sh.HW] = e[k] * (dp[k] - dot);
}

// ---------------------------------------------------------------------------------------------------------------- host side
template <typename F>
static inline void lov_by_class_bound(int K, F&& f) {
  if (K <= 8) f(std::integral_constant<int, 8>());
  else if (K <= 16) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, PLOV_MAX_K>());
}

static inline size_t lov_up8(size_t b) { return (b + 7) & ~(size_t)7; }

struct LovPlan {
  unsigned S, n, T;
  size_t total;
  size_t off_keys[2], off_pay[2], off_table, off_sums, off_tilefg, off_G, off_partial, off_segloss, bytes;
};

static LovPlan lov_plan(size_t S, size_t n, bool loss) {
  LovPlan p;
  p.S = (unsigned)S;
  p.n = (unsigned)n;
  p.T = (unsigned)((n + PLOV_TILE - 1) / PLOV_TILE);
  p.total = S * n;
  size_t at = 0;
  for (int i = 0; i < 2; ++i) {
    p.off_keys[i] = at;
    at += lov_up8(p.total * 4);
    p.off_pay[i] = at;
    at += lov_up8(p.total * 4);
  }
  p.off_table = at;
  at += lov_up8(S * PLOV_RADIX * (size_t)p.T * 4);
  p.off_sums = at;      // the chunks' sums of a long scan: the digit table has the most chunks
  at += lov_up8(S * ((PLOV_RADIX * (size_t)p.T + PLOV_SCAN_CHUNK - 1) / PLOV_SCAN_CHUNK) * 4);
  p.off_tilefg = p.off_G = p.off_partial = p.off_segloss = at;
  if (loss) {
    p.off_tilefg = at;
    at += lov_up8(S * (size_t)p.T * 4);
    p.off_G = at;
    at += lov_up8(S * 4);
    p.off_partial = at;
    at += S * (size_t)p.T * 8;
    p.off_segloss = at;
    at += S * 8;
  }
  p.bytes = at;
  return p;
}

// exclusive scan in place of the digit tables of S segments, `len` words each
static void lov_scan_table(unsigned* table, unsigned S, size_t len, unsigned* sums, hipStream_t st) {
  const dim3 block(PLOV_THREADS);
  if (len <= PLOV_SCAN_SHORT) {
    lov_scan_kernel<<<dim3(S), block, 0, st>>>(table, len, len, 1u, nullptr, nullptr);
    return;
  }
  const unsigned C = (unsigned)((len + PLOV_SCAN_CHUNK - 1) / PLOV_SCAN_CHUNK);
  lov_chunk_sum_kernel<<<dim3(S * C), block, 0, st>>>(table, len, (size_t)PLOV_SCAN_CHUNK, C, sums);
  lov_scan_kernel<<<dim3(S), block, 0, st>>>(sums, (size_t)C, (size_t)C, 1u, nullptr, nullptr);
  lov_scan_kernel<<<dim3(S * C), block, 0, st>>>(table, len, (size_t)PLOV_SCAN_CHUNK, C, sums, nullptr);
}

// the four passes; the sorted (key, payload) end where they began, in buffer 0
static int lov_sort(const LovPlan& p, char* ws, hipStream_t st, const char* who) {
  unsigned* keys[2] = {(unsigned*)(ws + p.off_keys[0]), (unsigned*)(ws + p.off_keys[1])};
  unsigned* pay[2] = {(unsigned*)(ws + p.off_pay[0]), (unsigned*)(ws + p.off_pay[1])};
  unsigned* table = (unsigned*)(ws + p.off_table);
  unsigned* sums = (unsigned*)(ws + p.off_sums);
  const dim3 grid(p.S * p.T), block(PLOV_THREADS);
  for (int pass = 0; pass < PLOV_PASSES; ++pass) {
    const int a = pass & 1, b = a ^ 1, shift = 8 * pass;
    lov_hist_kernel<<<grid, block, 0, st>>>(keys[a], p.n, p.T, shift, table);
    lov_scan_table(table, p.S, (size_t)PLOV_RADIX * p.T, sums, st);
    lov_scatter_kernel<<<grid, block, 0, st>>>(keys[a], pay[a], keys[b], pay[b], p.n, p.T, shift, table);
    const int rc = lov_launched(who);
    if (rc != 0) return rc;
  }
  return 0;
}

static int lov_check_sort_shape(const char* who, int S, int n) {
  LOV_CHECK_ARG(S >= 1 && n >= 1, "%s: S = %d, n = %d, need S >= 1 and n >= 1", who, S, n);
  LOV_CHECK_ARG((long long)S * n < (1ll << 31), "%s: S * n = %lld, need fewer than 2^31 keys", who, (long long)S * n);
  return 0;
}

static int lov_check_shape(const char* who, int N, int K, int H, int W) {
  LOV_CHECK_ARG(K >= PLOV_MIN_K && K <= PLOV_MAX_K, "%s: K = %d, need %d <= K <= %d", who, K, PLOV_MIN_K, PLOV_MAX_K);
  LOV_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "%s: N = %d, H = %d, W = %d, need all >= 1", who, N, H, W);
  // N * K * H * W < 2^31, without overflowing on the way
  LOV_CHECK_ARG((long long)H * W < (1ll << 31) && (long long)N * K < (1ll << 31) && (long long)N * K * ((long long)H * W) < (1ll << 31),
                "%s: N * K * H * W = %lld x %lld, need fewer than 2^31 elements", who, (long long)N * K, (long long)H * W);
  return 0;
}

static inline LovPlan lov_loss_plan(int N, int K, int H, int W, int per_image) {
  return per_image ? lov_plan((size_t)N * K, (size_t)H * W, true) : lov_plan((size_t)K, (size_t)N * H * W, true);
}

static inline LovShape lov_shape(int N, int K, int H, int W, int has_ignore, long long ignore_index, int per_image) {
  LovShape s;
  s.K = K;
  s.HW = H * W;
  s.per_image = per_image;
  s.has_ignore = has_ignore;
  s.ignore_index = ignore_index;
  s.total = (unsigned)((long long)N * H * W);
  return s;
}

extern "C" int plov_version(void) { return PLOV_VERSION; }
extern "C" const char* plov_last_error(void) { return g_lov_err; }
extern "C" int plov_tile(void) { return PLOV_TILE; }

extern "C" size_t plov_sort_workspace(int S, int n) {
  if (lov_check_sort_shape("plov_sort_workspace", S, n) != 0) return 0;
  return lov_plan((size_t)S, (size_t)n, false).bytes;
}

extern "C" int plov_sort_descending(const float* values, int S, int n, float* sorted, int* perm, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* who = "plov_sort_descending";
  LOV_CHECK_ARG(values && sorted && perm && workspace, "%s: null pointer (values %p, sorted %p, perm %p, workspace %p)", who,
                (const void*)values, (void*)sorted, (void*)perm, workspace);
  LOV_CHECK_ARG((((uintptr_t)values | (uintptr_t)sorted | (uintptr_t)perm) & 3) == 0, "%s: pointers must be 4-byte aligned", who);
  LOV_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  int rc = lov_check_sort_shape(who, S, n);
  if (rc != 0) return rc;
  const LovPlan p = lov_plan((size_t)S, (size_t)n, false);
  LOV_CHECK_ARG(workspace_bytes >= p.bytes, "%s: workspace of %zu bytes, need %zu (plov_sort_workspace)", who, workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const dim3 flat((unsigned)((p.total + PLOV_THREADS - 1) / PLOV_THREADS)), block(PLOV_THREADS);
  lov_float_key_kernel<<<flat, block, 0, st>>>(values, p.n, p.total, (unsigned*)(ws + p.off_keys[0]), (unsigned*)(ws + p.off_pay[0]));
  rc = lov_launched(who);
  if (rc != 0) return rc;
  rc = lov_sort(p, ws, st, who);
  if (rc != 0) return rc;
  lov_sort_finish_kernel<<<flat, block, 0, st>>>(values, (const unsigned*)(ws + p.off_pay[0]), p.n, p.total, sorted, perm);
  return lov_launched("plov_sort_descending (finish)");
}

extern "C" size_t plov_loss_workspace(int N, int K, int H, int W, int per_image) {
  if (lov_check_shape("plov_loss_workspace", N, K, H, W) != 0) return 0;
  return lov_loss_plan(N, K, H, W, per_image != 0).bytes;
}

extern "C" int plov_loss_fwd(const float* logits, const long long* target, int N, int K, int H, int W, int has_ignore,
                             long long ignore_index, int per_image, int classes_all, float* loss, float* weights, float* seg_scale,
                             float* errors, int* perm, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "plov_loss_fwd";
  LOV_CHECK_ARG(logits && target && loss && weights && seg_scale && workspace,
                "%s: null pointer (logits %p, target %p, loss %p, weights %p, seg_scale %p, workspace %p)", who, (const void*)logits,
                (const void*)target, (void*)loss, (void*)weights, (void*)seg_scale, workspace);
  LOV_CHECK_ARG((((uintptr_t)logits | (uintptr_t)loss | (uintptr_t)weights | (uintptr_t)seg_scale | (uintptr_t)errors | (uintptr_t)perm) & 3) == 0,
                "%s: pointers must be 4-byte aligned", who);
  LOV_CHECK_ARG((((uintptr_t)target | (uintptr_t)workspace) & 7) == 0, "%s: target and the workspace must be 8-byte aligned", who);
  int rc = lov_check_shape(who, N, K, H, W);
  if (rc != 0) return rc;
  LOV_CHECK_ARG((has_ignore == 0 || has_ignore == 1) && (per_image == 0 || per_image == 1) && (classes_all == 0 || classes_all == 1),
                "%s: has_ignore = %d, per_image = %d, classes_all = %d, need 0 or 1", who, has_ignore, per_image, classes_all);
  const LovPlan p = lov_loss_plan(N, K, H, W, per_image);
  LOV_CHECK_ARG(workspace_bytes >= p.bytes, "%s: workspace of %zu bytes, need %zu (plov_loss_workspace)", who, workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const LovShape sh = lov_shape(N, K, H, W, has_ignore, ignore_index, per_image);
  unsigned* keys = (unsigned*)(ws + p.off_keys[0]);
  unsigned* pay = (unsigned*)(ws + p.off_pay[0]);
  unsigned* tilefg = (unsigned*)(ws + p.off_tilefg);
  unsigned* G = (unsigned*)(ws + p.off_G);
  double* partial = (double*)(ws + p.off_partial);
  double* segloss = (double*)(ws + p.off_segloss);
  const dim3 pixels((sh.total + PLOV_THREADS - 1) / PLOV_THREADS), tiles(p.S * p.T), block(PLOV_THREADS);
  lov_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    lov_key_kernel<MK><<<pixels, block, 0, st>>>(logits, target, sh, keys, pay, errors);
  });
  rc = lov_launched(who);
  if (rc != 0) return rc;
  rc = lov_sort(p, ws, st, who);
  if (rc != 0) return rc;
  lov_fgcount_kernel<<<tiles, block, 0, st>>>(pay, p.n, p.T, tilefg);
  lov_scan_kernel<<<dim3(p.S), block, 0, st>>>(tilefg, (size_t)p.T, (size_t)p.T, 1u, nullptr, G);      // 1 / 256 of a digit table: one block
  lov_weight_kernel<<<tiles, block, 0, st>>>(keys, pay, p.n, p.T, tilefg, G, sh, weights, perm, partial);
  rc = lov_launched("plov_loss_fwd (weights)");
  if (rc != 0) return rc;
  lov_segsum_kernel<<<dim3((p.S + PLOV_WAVES - 1) / PLOV_WAVES), block, 0, st>>>(partial, p.S, p.T, segloss);
  lov_final_kernel<<<dim3(1), block, 0, st>>>(segloss, G, per_image ? (unsigned)N : 1u, K, classes_all, seg_scale, loss);
  return lov_launched("plov_loss_fwd (reduce)");
}

extern "C" int plov_loss_bwd(const float* logits, const long long* target, int N, int K, int H, int W, int has_ignore,
                             long long ignore_index, int per_image, const float* weights, const float* seg_scale, const float* grad,
                             float* dlogits, void* stream) {
  const char* who = "plov_loss_bwd";
  LOV_CHECK_ARG(logits && target && weights && seg_scale && grad && dlogits,
                "%s: null pointer (logits %p, target %p, weights %p, seg_scale %p, grad %p, dlogits %p)", who, (const void*)logits,
                (const void*)target, (const void*)weights, (const void*)seg_scale, (const void*)grad, (void*)dlogits);
  LOV_CHECK_ARG((((uintptr_t)logits | (uintptr_t)weights | (uintptr_t)seg_scale | (uintptr_t)grad | (uintptr_t)dlogits) & 3) == 0,
                "%s: pointers must be 4-byte aligned", who);
  LOV_CHECK_ARG(((uintptr_t)target & 7) == 0, "%s: target must be 8-byte aligned", who);
  const int rc = lov_check_shape(who, N, K, H, W);
  if (rc != 0) return rc;
  LOV_CHECK_ARG((has_ignore == 0 || has_ignore == 1) && (per_image == 0 || per_image == 1), "%s: has_ignore = %d, per_image = %d, need 0 or 1",
                who, has_ignore, per_image);
  const LovShape sh = lov_shape(N, K, H, W, has_ignore, ignore_index, per_image);
  lov_by_class_bound(K, [&](auto mk) {
    constexpr int MK = decltype(mk)::value;
    lov_bwd_kernel<MK><<<dim3((sh.total + PLOV_THREADS - 1) / PLOV_THREADS), dim3(PLOV_THREADS), 0, (hipStream_t)stream>>>(
        logits, target, sh, weights, seg_scale, grad, dlogits);
  });
  return lov_launched(who);
}
