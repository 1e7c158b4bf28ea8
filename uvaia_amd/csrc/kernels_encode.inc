// kernels_encode.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the inverse of kernels_expand.inc -- resident
// dense tiles encoded into the compact form of a packed database (version 2 of uvaia_amd/csrc/host/uvdb.h: per reference the 32-site words
// that differ from a base row, as fill and literal heads).  The encoding is the canonical one compact_encode_tiles (host/uvdb.c) writes.
//
// Three passes.  encode_count_kernel and encode_emit_kernel make the same walk (encode_walk): one wave per tile, lane = reference, the word
// groups in order.  The four plane rows of a word group are four coalesced 1 KiB wave loads, the base's four uint4 of the group are the same
// for every lane (scalar loads).  Each lane runs the open-head state machine of the host encoder in registers -- kind (0 none, 1 fill,
// 2 literal), code, first word, run length -- over the real words 0 .. n_real - 1 only: the padding words behind nchar are never looked at.
// A reference is never split over waves: runs merge across any cut and the encoding would no longer be canonical.  The count pass leaves a
// lane's number of heads and of literal words; encode_prefix_kernel turns both into 64-bit offsets relative to the call's first lane; the
// emit pass stores heads and literal words (uint4: planes A, C, G, T) at the lane's offsets, every store bounded by the extent the offsets
// give the lane, so a disagreement between the two walks cannot write outside it.  Lanes at and past n_valid (the lanes behind the last
// resident reference) are walked as all-zero rows whatever the tile holds there.

template <bool EMIT>
static __device__ __forceinline__ void encode_walk(const uint4 *__restrict__ tile, const uint4 *__restrict__ base, int n_real, bool zero_row,
                                                   uint32_t &nh, uint32_t &nl, uint32_t *__restrict__ heads, uint32_t max_h, uint4 *__restrict__ lits, uint32_t max_l)
{
  const int lane = threadIdx.x;
  uint32_t kind = 0, code = 0, first = 0, run = 0;
  nh = 0; nl = 0;
  const int groups = (n_real + 3) >> 2;
  for (int w4 = 0; w4 < groups; w4++) {
    uint4 x[4], b[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      x[p] = tile[(size_t)(w4 * 4 + p) * 64 + lane];
      b[p] = base[w4 * 4 + p];
      if (zero_row) x[p] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int word = w4 * 4 + j;
      if (word < n_real) {
        uint32_t v[4], k = 0, c = 0;
        bool differs = false;
#pragma unroll
        for (int p = 0; p < 4; p++) { v[p] = u4c(x[p], j); differs |= v[p] != u4c(b[p], j); }
        if (differs) {
          k = 1;
#pragma unroll
          for (int p = 0; p < 4; p++) { if (v[p] == 0xFFFFFFFFu) c |= 1u << p; else if (v[p]) k = 2; }
          if (k == 2) c = 0;
        }
        if (!k || k != kind || c != code || run == 2047u) {
          if (kind) {
            if (EMIT && nh < max_h) heads[nh] = (first << 16) | (run << 5) | ((kind == 2 ? 1u : 0u) << 4) | code;
            nh++;
          }
          kind = k; code = c; first = (uint32_t)word; run = 0;
        }
        if (k) run++;
        if (k == 2) {
          if (EMIT && nl < max_l) lits[nl] = make_uint4(v[0], v[1], v[2], v[3]);
          nl++;
        }
      }
    }
  }
  if (kind) {
    if (EMIT && nh < max_h) heads[nh] = (first << 16) | (run << 5) | ((kind == 2 ? 1u : 0u) << 4) | code;
    nh++;
  }
}

// tiles: the first tile of the call; n_valid: lanes of the call that hold a reference; cnt_h / cnt_l: 64 * gridDim.x counts
__global__ __launch_bounds__(64) void encode_count_kernel(const uint4 *__restrict__ tiles, const uint4 *__restrict__ base, int W4, int n_real, unsigned long long n_valid,
                                                           uint32_t *__restrict__ cnt_h, uint32_t *__restrict__ cnt_l)
{
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  uint32_t nh, nl;
  encode_walk<false>(tiles + (size_t)blockIdx.x * W4 * 4 * 64, base, n_real, g >= n_valid, nh, nl, nullptr, 0u, nullptr, 0u);
  cnt_h[g] = nh; cnt_l[g] = nl;
}

// Exclusive prefix sums of both count arrays: idx[0] = 0, idx[g + 1] = idx[g] + cnt[g], n + 1 entries each.  ONE block walks the lanes in
// chunks of its 1024 threads and carries the totals from chunk to chunk, so the result does not depend on how many lanes a block holds: a
// wave scan by __shfl_up, the 16 wave totals through LDS, the carry in a register of every thread.  The pass reads 8 bytes per lane where the
// count pass reads a reference's planes: one block does not show.
__global__ __launch_bounds__(1024) void encode_prefix_kernel(const uint32_t *__restrict__ cnt_h, const uint32_t *__restrict__ cnt_l, unsigned long long n,
                                                              unsigned long long *__restrict__ hidx, unsigned long long *__restrict__ lidx)
{
  __shared__ unsigned long long tot[2][16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long carry_h = 0, carry_l = 0;
  if (threadIdx.x == 0) { hidx[0] = 0; lidx[0] = 0; }
  for (unsigned long long a = 0; a < n; a += 1024) {
    const unsigned long long g = a + threadIdx.x;
    unsigned long long h = g < n ? cnt_h[g] : 0u, l = g < n ? cnt_l[g] : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long uh = __shfl_up(h, d), ul = __shfl_up(l, d);
      if (lane >= d) { h += uh; l += ul; }
    }
    if (lane == 63) { tot[0][wv] = h; tot[1][wv] = l; }
    __syncthreads();
    unsigned long long before_h = carry_h, before_l = carry_l, all_h = 0, all_l = 0;
#pragma unroll
    for (int v = 0; v < 16; v++) {
      if (v < wv) { before_h += tot[0][v]; before_l += tot[1][v]; }
      all_h += tot[0][v]; all_l += tot[1][v];
    }
    if (g < n) { hidx[g + 1] = before_h + h; lidx[g + 1] = before_l + l; }
    carry_h += all_h; carry_l += all_l;
    __syncthreads();
  }
}

// heads / lits: where the call's records start; a lane's extent is [idx[g], idx[g + 1])
__global__ __launch_bounds__(64) void encode_emit_kernel(const uint4 *__restrict__ tiles, const uint4 *__restrict__ base, int W4, int n_real, unsigned long long n_valid,
                                                          const unsigned long long *__restrict__ hidx, const unsigned long long *__restrict__ lidx,
                                                          uint32_t *__restrict__ heads, uint4 *__restrict__ lits)
{
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const unsigned long long hb = hidx[g], he = hidx[g + 1], lb = lidx[g], le = lidx[g + 1];
  const uint32_t max_h = he > hb ? (uint32_t)min(he - hb, 0xFFFFFFFFull) : 0u, max_l = le > lb ? (uint32_t)min(le - lb, 0xFFFFFFFFull) : 0u;
  uint32_t nh, nl;
  encode_walk<true>(tiles + (size_t)blockIdx.x * W4 * 4 * 64, base, n_real, g >= n_valid, nh, nl, heads + hb, max_h, lits + lb, max_l);
}
