// uvaia_cluster.hip -- MI355X (gfx950 / CDNA4) one-pass canopy clustering behind include/uvaia_cluster.h (`uvaiaclust`).
//
// What it replaces in the reference: phase 2 of src/cluster.c:163-205 (check_seq_against_cluster, src/fastaseq.c:140-170, under
// "#pragma omp parallel for" over the queues) and the merge tree of src/cluster.c:216-233 (merge_clusters, src/fastaseq.c:196-258).
// The semantics are those the header states (the reference's code, not its comments); DESIGN.md "uvaiaclust" has the derivation.
//
// Design:
//   * every pushed row stays resident (pitch padded to 64 B with zero bytes, which never differ).  A lane compares 16 B per load:
//     the mismatching bytes of a 32-bit word are the high bits of ((x & 0x7f..) + 0x7f.. | x) & 0x80.. with x = a ^ b, counted by
//     v_bcnt.  A wave compares 4 KB per round trip and stops once its count passes the distance.
//   * prep: one wave per pushed row.  It upper-cases the row in place, flags bytes 0 and >= 0x80, counts the differences from the
//     reference over the trimmed sites and records the first n_score of them (ballot-free: a wave prefix sum of the per-lane counts).
//   * queue: one workgroup of four waves per queue, for the rows of one push in queue order.  The stored distances of the queue's
//     medoids live in LDS (global memory past LDS_ST of them).  Wave 0 collects the next four candidates of the ordered candidate
//     list (header, item 3) by ballots over the stored distances, each wave compares one of them, and the lowest matching wins.
//   * merge: one launch per round of the tree, one wave per (pair, absorbed cluster): the host gives each its window of the
//     absorbing list (binary search on the sorted stored distances), the wave compares in order and stops at the first match.
//     The host does the stable sorts and splices the member lists.
//   * packed pushes (uvaia_clust_push_packed): the rows come as whole tiles of the packed interchange form and are rebuilt on the device.
//     unpack: lane = reference, one 1 KiB wave load per plane and word group, sets decoded to characters in registers (iupac_decode.h), a
//     transpose through an XOR-swizzled LDS image so that every row's 128 characters of a word group leave as eight 16-byte stores.
//     overlay: the exception runs ('-', '?', 'X', 'O', '.': the planes hold them all as the empty set) are written over the decoded rows,
//     one wave per run, the lanes spread over its length.  Prep and queue then run on these rows as on rows that came as text.
//   * device pushes (uvaia_clust_push_device): the rows come as text that is already in device memory (what the FASTA parser leaves behind,
//     uvaia_gpu_fasta_rows), at any pitch and alignment.  rows_in: one block per row copies its nchar bytes to the store or the staging row
//     and pads it with zero bytes, as the host's copy of uvaia_clust_push does; prep and queue then run as on any other push.
//   * keep medoids (uvaia_clust_keep_medoids): the second residency mode.  A row is read again after phase 2 has placed it only if it
//     founded a cluster, so only founders are kept: the rows of a push land in a staging buffer, the queue kernel reads the row it places
//     and the founders of the running push from staging and earlier founders from their slot, and after it the founders of the push get
//     consecutive slots in push order (a block-wise prefix sum over join[] < 0) and their rows are copied to the slots.  Slots live in slabs
//     of slab_rows rows (a power of two) behind a device table of base pointers: growth adds a slab and copies nothing.  The kernels that
//     read rows take the addressing as a template parameter (FlatRows / SlabRows); dist[], p[] and join[] stay per push ordinal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvaia_cluster.h"
#include "iupac_decode.h"
#include "rows_block.h"

namespace {

constexpr int QTPB = 256;               // queue kernel: four waves, one candidate each
constexpr int QW = QTPB / 64;
constexpr int LDS_ST = 14336;           // stored distances of a queue's first medoids kept in LDS (56 KB)
constexpr int PTPB = 256;               // prep and merge: one wave per row / item
constexpr int UNROLL = 4;               // 16-B loads in flight per lane in a comparison: 4 KB per wave per round trip
constexpr int UTPB = 256;               // unpack: four waves, each with a transpose image of its own (4 x 8 KiB of LDS)
constexpr int UGROUPS = 16;             // unpack: word groups per work unit (a 29 903-site alignment is 15 units per tile)
constexpr int OTPB = 256;               // overlay: one block per row, one wave per run
constexpr int RTPB = 256;               // rows in: one block per row, 16 sites per thread
constexpr int KTPB = 256;               // keep medoids: rows of a push per block of the founder prefix sum
constexpr int SLAB_ROWS = 65536;        // keep medoids: default rows per slab (1.96 GB at 29 952 B per row); a design choice, not measured

__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
__device__ __forceinline__ uint32_t expand4(uint32_t b) { return ((b & 1u) << 7) | ((b & 2u) << 14) | ((b & 4u) << 21) | ((b & 8u) << 28); }
__device__ __forceinline__ uint32_t pack4(uint32_t m) { return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u); }

// bytes j of the 16-byte chunk at pos with lo <= pos + j < hi
__device__ __forceinline__ uint32_t window16(int pos, int lo, int hi)
{
  const int a = max(lo - pos, 0), b = min(hi - pos, 16);
  return b <= a ? 0u : (((1u << b) - 1u) & ~((1u << a) - 1u));
}

// 16-bit mask of the bytes that differ between two 16-byte chunks, inside the window w16
__device__ __forceinline__ uint32_t diff_mask16(uint4 a, uint4 b, uint32_t w16)
{
  const uint32_t m = pack4(nz_bytes(a.x ^ b.x)) | (pack4(nz_bytes(a.y ^ b.y)) << 4) | (pack4(nz_bytes(a.z ^ b.z)) << 8) | (pack4(nz_bytes(a.w ^ b.w)) << 12);
  return m & w16;
}

__device__ __forceinline__ int diff_count16(uint4 a, uint4 b, uint32_t w16)
{
  if (w16 == 0xffffu)
    return __popc(nz_bytes(a.x ^ b.x)) + __popc(nz_bytes(a.y ^ b.y)) + __popc(nz_bytes(a.z ^ b.z)) + __popc(nz_bytes(a.w ^ b.w));
  return __popc(nz_bytes(a.x ^ b.x) & expand4(w16)) + __popc(nz_bytes(a.y ^ b.y) & expand4(w16 >> 4)) +
         __popc(nz_bytes(a.z ^ b.z) & expand4(w16 >> 8)) + __popc(nz_bytes(a.w ^ b.w) & expand4(w16 >> 12));
}

__device__ __forceinline__ int wave_sum(int v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Differences between rows a and b over the sites [lo, hi), by one wave; stops once the count passes limit (the value returned is
// then some count above limit).  Rows are 16-byte aligned and padded to a multiple of 64 bytes, hi <= the row's length.
__device__ int wave_distance(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int lo, int hi, int limit)
{
  const int lane = threadIdx.x & 63;
  int total = 0;
  for (int base = lo & ~15; base < hi; base += 64 * 16 * UNROLL) {
    uint4 x[UNROLL], y[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const int pos = base + (u * 64 + lane) * 16;
      if (pos < hi) { x[u] = *(const uint4 *)(a + pos); y[u] = *(const uint4 *)(b + pos); }
      else { x[u] = make_uint4(0, 0, 0, 0); y[u] = x[u]; }
    }
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const int pos = base + (u * 64 + lane) * 16;
      cnt += diff_count16(x[u], y[u], window16(pos, lo, hi));
    }
    total += wave_sum(cnt);
    if (total > limit) break;
  }
  return total;
}

// Where the kernels below find a row.  FlatRows: every pushed row stays, row o at rows + o * pitch.
struct FlatRows {
  const uint8_t *__restrict__ rows; size_t pitch;
  __device__ __forceinline__ const uint8_t *pushed(int o) const { return rows + (size_t)o * pitch; }
  __device__ __forceinline__ const uint8_t *by_ordinal(int o) const { return pushed(o); }
  __device__ __forceinline__ const uint8_t *medoid(int m, int, int, int) const { return pushed(m); }
  __device__ __forceinline__ void found(int, int, int, int) const {}
};

// SlabRows (keep medoids): the rows of the running push (ordinals first ..) in staging, founders of earlier pushes in their slots.
// m_loc (cap entries per queue, beside m_ord / m_st) says where a queue's medoid lies: its slot when >= 0, -1 - staging index for a
// founder of the running push; slot_of[o] is the slot of founder o of an earlier push (-1 for a row that joined).
struct SlabRows {
  const uint8_t *stage; uint8_t *const *slab; size_t pitch; const int *slot_of; int *m_loc; long long first; int shift, mask;
  __device__ __forceinline__ const uint8_t *kept(int slot) const { return slab[slot >> shift] + (size_t)(slot & mask) * pitch; }
  __device__ __forceinline__ const uint8_t *pushed(int o) const { return stage + (size_t)(o - first) * pitch; }
  __device__ __forceinline__ const uint8_t *by_ordinal(int o) const { return kept(slot_of[o]); }
  __device__ __forceinline__ const uint8_t *medoid(int, int q, int cap, int idx) const
  {
    const int l = m_loc[(size_t)q * cap + idx];
    return l >= 0 ? kept(l) : stage + (size_t)(-1 - l) * pitch;
  }
  __device__ __forceinline__ void found(int q, int cap, int idx, int o) const { m_loc[(size_t)q * cap + idx] = -1 - (int)(o - first); }
};

// One wave per pushed row (ordinals first .. first + n): upper-case in place, flag bytes 0 and >= 0x80 (bad_out = lowest such
// row of the push), distance to the reference over [trim, nchar - trim) and the first n_score differing sites (relative to trim).
__global__ __launch_bounds__(PTPB) void clust_prep_kernel(uint8_t *__restrict__ rows, size_t pitch, long long first, int n, const uint8_t *__restrict__ ref, int nchar,
                                                          int trim, int n_score, int *__restrict__ dist_out, int *__restrict__ p_out, int *__restrict__ bad_out)
{
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (PTPB / 64) + (threadIdx.x >> 6);
  if (w >= n) return;
  const long long o = first + w;
  uint8_t *row = rows + (size_t)o * pitch;
  int *p = p_out + (size_t)o * n_score;
  const int lo = trim, hi = nchar - trim;
  int total = 0;
  uint32_t bad = 0;
  for (int base = 0; base < nchar; base += 64 * 16) {
    const int pos = base + lane * 16;
    uint32_t dm = 0;
    if (pos < nchar) {
      uint4 v = *(uint4 *)(row + pos);
      const uint4 r = *(const uint4 *)(ref + pos);
      const uint32_t vw = window16(pos, 0, nchar);
      uint32_t *vv = &v.x;
      uint32_t lower_any = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t x = vv[k], in = expand4(vw >> (4 * k));
        bad |= ((~nz_bytes(x) & 0x80808080u) | (x & 0x80808080u)) & in;          // a zero byte, or one >= 0x80
        const uint32_t lower = (x + 0x1f1f1f1fu) & ~(x + 0x05050505u) & ~x & 0x80808080u & in;   // 'a'..'z' (no carries for bytes < 0x80)
        vv[k] = x - (lower >> 2);
        lower_any |= lower;
      }
      if (lower_any) *(uint4 *)(row + pos) = v;
      dm = diff_mask16(v, r, window16(pos, lo, hi));
    }
    const int cnt = __popc(dm);
    if (total < n_score) {            // wave-uniform: where the first n_score differences fall
      int incl = cnt;
      for (int s = 1; s < 64; s <<= 1) { const int t = __shfl_up(incl, s, 64); if (lane >= s) incl += t; }
      int rank = total + incl - cnt;
      for (uint32_t m = dm; m && rank < n_score; m &= m - 1, rank++) p[rank] = pos + __ffs(m) - 1 - trim;
    }
    total += wave_sum(cnt);
  }
  if (lane == 0) {
    dist_out[o] = total;
    for (int k = total; k < n_score; k++) p[k] = -1;
  }
  if (__ballot(bad != 0) && lane == 0) atomicMin(bad_out, w);
}

// Phase 2 for the rows of one push: workgroup q takes the ordinals qlist[qoff[q] .. qoff[q + 1]) in order against queue q's medoids
// (m_ord / m_st: cap slots per queue, m_count of them used).  join[o] = slot of the medoid o joined, or -1 - slot if o founded one.
// Rows says where the row being placed and a candidate's row lie (FlatRows: the code as it was before the parameter).
template <class Rows>
__global__ __launch_bounds__(QTPB) void clust_queue_kernel(const Rows rows, int nchar, int trim, int d, int n_score,
                                                           const int *__restrict__ dist, const int *__restrict__ p, const int *__restrict__ qoff,
                                                           const int *__restrict__ qlist, int *__restrict__ m_count, int *__restrict__ m_ord_all,
                                                           int *__restrict__ m_st_all, int cap, int *__restrict__ join)
{
  __shared__ int st[LDS_ST];
  __shared__ int cand[QW], hit[QW];
  __shared__ int s_ncand, s_next, s_after;
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = qoff[q], k1 = qoff[q + 1];
  if (k0 == k1) return;
  int *m_ord = m_ord_all + (size_t)q * cap, *m_st = m_st_all + (size_t)q * cap;
  int n = m_count[q];
  for (int i = threadIdx.x; i < min(n, LDS_ST); i += QTPB) st[i] = m_st[i];
  __syncthreads();
  const int d2 = 2 * d + 1;

  for (int k = k0; k < k1; k++) {
    const int o = qlist[k];
    const int r = dist[o];
    const int ps = n_score ? p[(size_t)o * n_score] : 0;
    int pos = 0, winner = -1;
    bool compared = false;
    if (threadIdx.x == 0) s_after = 0;
    __syncthreads();
    while (pos < n) {
      if (wave == 0) {   // the next QW candidates in list order: the first medoid within the ring of r, then those with 1 <= stored <= 2d + 1
        int got = 0, i = pos, last = pos;
        bool after = s_after != 0;
        while (got < QW && i < n) {
          const int idx = i + lane;
          bool pred = false;
          if (idx < n) {
            const int s = idx < LDS_ST ? st[idx] : m_st[idx];
            pred = after ? (s >= 1 && s <= d2) : (abs(r - s) <= d);
          }
          unsigned long long m = __ballot(pred);
          if (!m) { i += 64; continue; }
          if (!after) {
            const int b = __ffsll(m) - 1;
            if (lane == 0) cand[got] = i + b;
            got++; after = true; i = i + b + 1;
            continue;
          }
          while (m && got < QW) { const int b = __ffsll(m) - 1; if (lane == 0) cand[got] = i + b; got++; last = i + b; m &= m - 1; }
          i = got == QW ? last + 1 : i + 64;
        }
        if (lane == 0) { s_ncand = got; s_next = i; s_after = after; }
      }
      __syncthreads();
      const int nc = s_ncand;
      if (nc == 0) break;
      compared = true;
      if (wave < nc) {
        const int slot = cand[wave];
        const int m = m_ord[slot];
        int minloc = 0;
        if (n_score) minloc = max(0, min(ps, p[(size_t)m * n_score]) - 1);
        const int lo = trim + minloc, hi = min(nchar, nchar - trim + minloc);
        const int dd = wave_distance(rows.pushed(o), rows.medoid(m, q, cap, slot), lo, hi, d);
        if (lane == 0) hit[wave] = dd <= d;
      }
      __syncthreads();
      for (int w = 0; w < nc; w++) if (hit[w]) { winner = cand[w]; break; }
      pos = s_next;
      __syncthreads();     // cand / hit / s_next are rewritten by the next round
      if (winner >= 0) break;
    }
    if (winner >= 0) {
      if (threadIdx.x == 0) join[o] = winner;
    } else {
      if (threadIdx.x == 0) {
        const int stored = compared ? d + 1 : r;
        m_ord[n] = o; m_st[n] = stored;
        rows.found(q, cap, n, o);
        if (n < LDS_ST) st[n] = stored;
        join[o] = -1 - n;
      }
      n++;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (threadIdx.x == 0) m_count[q] = n;
}

// One wave per item of a merge round: item i compares row item_ord[i] with the rows list_ord[item_lo[i] .. item_hi[i]) in order over
// the trimmed sites and writes the first position within d (or -1) to target[i].
template <class Rows>
__global__ __launch_bounds__(PTPB) void clust_merge_kernel(const Rows rows, int nchar, int trim, int d, const int *__restrict__ item_ord,
                                                           const int *__restrict__ item_lo, const int *__restrict__ item_hi, const int *__restrict__ list_ord,
                                                           int n_items, int *__restrict__ target)
{
  const int w = blockIdx.x * (PTPB / 64) + (threadIdx.x >> 6);
  if (w >= n_items) return;
  const uint8_t *a = rows.by_ordinal(item_ord[w]);
  int t = -1;
  for (int j = item_lo[w], e = item_hi[w]; j < e; j++)
    if (wave_distance(a, rows.by_ordinal(list_ord[j]), trim, nchar - trim, d) <= d) { t = j; break; }
  if ((threadIdx.x & 63) == 0) target[w] = t;
}

// Byte offset of the 16-byte piece k (0..7) of row r (0..63) in a wave's transpose image: 64 rows of 128 B, piece index XORed with r & 7.
// Writes are lane = row, one piece index per instruction: ds_write_b128 is served in groups of 8 consecutive lanes over 32 banks (128 B), and
// the XOR sends those 8 rows to the 8 different 16-byte slots.  Reads are lane = (row 8 i + lane / 8, piece lane % 8): ds_read_b128 is served
// in four groups of 16 lanes over 64 banks (256 B = two rows); each group holds four rows, two even and two odd, with pieces {0-3} of one and
// {4-7} of the other of each parity, which the XOR permutes inside their halves: 16 different slots.  Every access stays 16-byte aligned.
__device__ __forceinline__ int unpack_image_offset(int r, int k) { return r * 128 + ((k ^ (r & 7)) << 4); }

// Whole tiles of the packed interchange form ([word group][plane A,C,G,T][lane] 16-byte words) -> rows of text.  Block = (tile, UGROUPS word
// groups of it), wave v of it takes the word groups g0 + v, g0 + v + 4, ...  Lane r loads the four plane words of reference r of the tile (1 KiB
// per wave load), decodes its 128 sites to characters and writes them to the wave's LDS image; the wave then stores 8 rows x 128 B per
// instruction.  rows points at the row of lane 0 of tile 0; lanes at and past n_ref are not written; sites in [nchar, pitch) are written as
// zero bytes (pitch is a multiple of 64: a piece starts below it or not at all).
__global__ __launch_bounds__(UTPB) void clust_unpack_tiles_kernel(const uint4 *__restrict__ tiles, int W4, int nchar, int n_ref, uint8_t *__restrict__ rows, size_t pitch,
                                                                  int units_per_tile)
{
  __shared__ uint4 image[UTPB / 64][64 * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x / units_per_tile, g0 = (blockIdx.x % units_per_tile) * UGROUPS, g1 = min(W4, g0 + UGROUPS);
  const uint4 *t = tiles + (size_t)tile * W4 * 4 * 64 + lane;
  uint8_t *im = reinterpret_cast<uint8_t *>(image[wave]);
  uint8_t *out = rows + (size_t)tile * 64 * pitch;
  const int live = min(64, n_ref - tile * 64);
  for (int base = g0; base < g1; base += UTPB / 64) {
    const int w4 = base + wave;
    if (w4 < g1) {
      const uint4 *p = t + (size_t)w4 * 4 * 64;
      const uint4 pa = p[0], pc = p[64], pg = p[128], pt = p[192];
      const uint32_t A[4] = {pa.x, pa.y, pa.z, pa.w}, C[4] = {pc.x, pc.y, pc.z, pc.w}, G[4] = {pg.x, pg.y, pg.z, pg.w}, T[4] = {pt.x, pt.y, pt.z, pt.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        uint32_t o[8];
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = iupac_text4((A[j] >> (4 * q)) & 15u, (C[j] >> (4 * q)) & 15u, (G[j] >> (4 * q)) & 15u, (T[j] >> (4 * q)) & 15u);
        *reinterpret_cast<uint4 *>(im + unpack_image_offset(lane, 2 * j)) = make_uint4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<uint4 *>(im + unpack_image_offset(lane, 2 * j + 1)) = make_uint4(o[4], o[5], o[6], o[7]);
      }
    }
    __syncthreads();
    const int k = lane & 7, site0 = w4 * 128 + k * 16;
    if (w4 < g1 && site0 < (int)pitch) {
      const int keep = nchar - site0;                  // characters of this piece inside the alignment
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int r = i * 8 + (lane >> 3);
        if (r >= live) continue;
        uint4 v = *reinterpret_cast<const uint4 *>(im + unpack_image_offset(r, k));
        if (keep < 16) {
          uint32_t *vv = &v.x;
#pragma unroll
          for (int m = 0; m < 4; m++) { const int kb = min(max(keep - 4 * m, 0), 4); vv[m] &= kb == 4 ? 0xffffffffu : ((1u << (8 * kb)) - 1u); }
        }
        *reinterpret_cast<uint4 *>(out + (size_t)r * pitch + site0) = v;
      }
    }
    __syncthreads();     // the image is rewritten by the next round
  }
}

// The exception runs of a push over its decoded rows.  Block i = row i of the push (rows points at it); its records are rec[off[i] .. off[i + 1]),
// (pos, len << 8 | char), checked by the host: inside the row, in increasing position, not overlapping.  One wave per record, the lanes spread
// over its length in aligned 4-byte words; the words a run covers partly are written byte by byte, so neighbouring runs never touch each other.
__global__ __launch_bounds__(OTPB) void clust_overlay_runs_kernel(uint8_t *__restrict__ rows, size_t pitch, const uint32_t *__restrict__ off, const uint2 *__restrict__ rec)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t *row = rows + (size_t)blockIdx.x * pitch;
  for (uint32_t e = off[blockIdx.x] + wave, e1 = off[blockIdx.x + 1]; e < e1; e += OTPB / 64) {
    const uint2 x = rec[e];
    const uint32_t pos = x.x, len = x.y >> 8, ch = x.y & 0xffu, end = pos + len;
    if (!len) continue;
    for (uint32_t w = (pos >> 2) + lane, w1 = (end - 1) >> 2; w <= w1; w += 64) {
      const uint32_t s = 4 * w;
      if (s >= pos && s + 4 <= end) *reinterpret_cast<uint32_t *>(row + s) = ch * 0x01010101u;
      else for (uint32_t b = s; b < s + 4; b++) if (b >= pos && b < end) row[b] = (uint8_t)ch;
    }
  }
}

// uvaia_clust_push_device: block i copies row row_index[i] (NULL: row i) of a block of text rows in device memory -- `pitch` bytes apart, no
// alignment assumed -- to row i of dst (the place of the push in the store, or the staging buffer: 16-byte aligned, dst_pitch a multiple of
// 64).  16 sites per thread (rows_block.h: one dwordx4 load where the source piece is aligned, five aligned dwords otherwise; no dword is
// touched that holds no byte of the row), one dwordx4 store each; the bytes from nchar to dst_pitch are zero, which never differ.
__global__ __launch_bounds__(RTPB) void clust_rows_in_kernel(const uint8_t *__restrict__ rows, size_t pitch, int nchar, const int *__restrict__ row_index,
                                                             uint8_t *__restrict__ dst, size_t dst_pitch)
{
  const int r = row_index ? row_index[blockIdx.x] : (int)blockIdx.x;
  const uint8_t *row = rows + (size_t)r * pitch;
  uint4 *out = reinterpret_cast<uint4 *>(dst + (size_t)blockIdx.x * dst_pitch);
  const int n16 = (int)(dst_pitch >> 4);
  for (int t = threadIdx.x; t < n16; t += RTPB)
    out[t] = (t * 16 < nchar) ? rows_load16_fill<0u>(row, nchar, t * 16) : make_uint4(0u, 0u, 0u, 0u);
}

// uvaia_clust_rows: row k of dst = row ord[k] of the store (whole pitch, 16 bytes per thread)
template <class Rows>
__global__ __launch_bounds__(256) void clust_gather_rows_kernel(const Rows rows, const int *__restrict__ ord, uint8_t *__restrict__ dst)
{
  const size_t pitch = rows.pitch;
  const uint4 *s = reinterpret_cast<const uint4 *>(rows.by_ordinal(ord[blockIdx.x]));
  uint4 *d = reinterpret_cast<uint4 *>(dst + (size_t)blockIdx.x * pitch);
  for (int k = threadIdx.x; k < (int)(pitch / 16); k += 256) d[k] = s[k];
}

// Keep medoids, after the queue kernel of a push of n rows (ordinals first ..): the founders (join < 0) get the slots kept, kept + 1, ... in
// push order.  Three steps, so that a push of any size works: founders per block of KTPB rows; the exclusive prefix sum of those counts by one
// block (blk[nb] = all founders of the push, which the host reads to add slabs before the next step); then every row's slot.
__global__ __launch_bounds__(KTPB) void clust_founder_count_kernel(const int *__restrict__ join, long long first, int n, int *__restrict__ blk)
{
  __shared__ int s[KTPB / 64];
  const int i = blockIdx.x * KTPB + threadIdx.x;
  const int cnt = __popcll(__ballot(i < n && join[first + i] < 0));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < KTPB / 64; w++) t += s[w]; blk[blockIdx.x] = t; }
}

__global__ __launch_bounds__(KTPB) void clust_founder_offsets_kernel(int *__restrict__ blk, int nb)
{
  __shared__ int s[KTPB / 64];
  __shared__ int carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += KTPB) {
    const int i = base + threadIdx.x, v = i < nb ? blk[i] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    if (lane == 63) s[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; w++) before += s[w];
    if (i < nb) blk[i] = before + incl - v;
    __syncthreads();                 // every thread has read carry and s
    if (threadIdx.x == KTPB - 1) carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) blk[nb] = carry;
}

// slot_of[o] = the slot of founder o, -1 for a row that joined; the founder's entry of its queue's m_loc (queue pq[i], list position
// -1 - join[o]) goes from its staging index to the slot.
__global__ __launch_bounds__(KTPB) void clust_founder_slots_kernel(const int *__restrict__ join, const int *__restrict__ pq, long long first, int n, const int *__restrict__ blk,
                                                                   int kept, int *__restrict__ slot_of, int *__restrict__ m_loc, int cap)
{
  __shared__ int s[KTPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * KTPB + threadIdx.x;
  const int j = i < n ? join[first + i] : 0;
  const unsigned long long m = __ballot(j < 0);
  if (lane == 0) s[wave] = __popcll(m);
  __syncthreads();
  int before = blk[blockIdx.x];
  for (int w = 0; w < wave; w++) before += s[w];
  if (i >= n) return;
  const int slot = j < 0 ? kept + before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
  slot_of[first + i] = slot;
  if (j < 0) m_loc[(size_t)pq[i] * cap + (-1 - j)] = slot;
}

// block i: row i of staging to its slot if it founded a cluster (whole pitch, 16 bytes per thread)
__global__ __launch_bounds__(256) void clust_keep_founders_kernel(const uint8_t *__restrict__ stage, size_t pitch, long long first, const int *__restrict__ slot_of,
                                                                  uint8_t *const *__restrict__ slab, int shift, int mask)
{
  const int slot = slot_of[first + blockIdx.x];
  if (slot < 0) return;
  const uint4 *s = reinterpret_cast<const uint4 *>(stage + (size_t)blockIdx.x * pitch);
  uint4 *d = reinterpret_cast<uint4 *>(slab[slot >> shift] + (size_t)(slot & mask) * pitch);
  for (int k = threadIdx.x; k < (int)(pitch / 16); k += 256) d[k] = s[k];
}

thread_local std::string g_open_error;

}  // namespace

// ---- host side.  Device memory, events and the stream are the move-only handles of host_owners.h; a failed HIP call goes through hip_failed.
struct uvaia_clust_ctx;
namespace { int hip_failed(uvaia_clust_ctx *c, hipError_t e, const char *call, const char *file, int line); }
#include <memory>
#include "host_owners.h"

// Members are destroyed last to first: the stream comes first so that it outlives every buffer and event that work queued on it may still
// name (uvaia_clust_close has waited for it by then).
struct uvaia_clust_ctx {
  Stream stream;
  Event ev_a, ev_b;
  int device = 0, nchar = 0, dist = 0, trim = 0, n_score = 0, n_queues = 0;
  size_t pitch = 0;
  DevBuf<uint8_t> d_ref, d_rows;
  DevBuf<int> d_dist, d_p, d_join, d_bad;                  // d_rows (or d_slot), d_dist, d_p and d_join hold rows_cap rows
  DevBuf<int> d_qoff, d_qlist, d_mcount, d_mord, d_mst;    // d_mord, d_mst (and d_mloc): m_cap slots per queue
  DevBuf<uint8_t> d_tiles, d_gather;                       // packed pushes: the tiles of a push; uvaia_clust_rows: the gathered rows
  DevBuf<uint32_t> d_xoff; DevBuf<uint2> d_xrec;           // packed pushes: record offsets per row of the push, and the records
  DevBuf<int> d_gord, d_rsel;                              // the ordinals of a gather; device pushes: the rows selected from the caller's block
  size_t rows_cap = 0;
  int m_cap = 0;
  long long pushed = 0;
  // keep medoids: the rows of the running push (d_stage, exactly as large as the largest push), the founders in slabs (slabs / d_slabtab), and where they are
  bool keep = false;
  int slab_rows = 0, slab_shift = 0;
  std::vector<DevBuf<uint8_t>> slabs;
  DevBuf<uint8_t *> d_slabtab; DevBuf<uint8_t> d_stage;
  DevBuf<int> d_slot, d_mloc, d_blk, d_pq;   // slot per push ordinal, location per medoid entry, prefix-sum scratch, queue per row of the push
  long long kept = 0;                      // founders so far = slots in use
  std::vector<int> h_slot;                 // d_slot on the host: uvaia_clust_rows and uvaia_clust_gather_device check their ordinals against it
  size_t peak_row_bytes = 0;
  std::vector<long long> per_queue;        // rows pushed to each queue so far (bounds its medoid count)
  std::vector<int> queue_of;               // queue of every pushed row
  std::vector<uint8_t> h_rows;
  std::vector<uint32_t> h_xoff;
  double prep_ms = 0, queue_ms = 0, merge_ms = 0, decode_ms = 0, overlay_ms = 0, rows_in_ms = 0;
  bool finished = false, broken = false;
  // after finish: clusters in the final order
  std::vector<long long> r_medoid, r_offsets, r_members;
  std::vector<int> r_scores;
  std::string err;
};

namespace {

int cfail(uvaia_clust_ctx *c, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (c) c->err = buf; else g_open_error = buf;
  return code;
}

// a failed HIP call leaves the context unusable (c is null while uvaia_clust_open builds it: the message goes where uvaia_clust_last_error(NULL) finds it)
int hip_failed(uvaia_clust_ctx *c, hipError_t e, const char *call, const char *file, int line)
{
  if (c) c->broken = true;
  return cfail(c, e == hipErrorOutOfMemory ? UVAIA_GPU_ENOMEM : UVAIA_GPU_EHIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
}

// what every entry point that works on the device asks first
int usable(uvaia_clust_ctx *c)
{
  return c->broken ? cfail(c, UVAIA_GPU_ESTATE, "context unusable after an earlier error: %s", c->err.c_str()) : 0;
}

// a device scratch array of at least n elements whose contents are not kept: kernels queued on the stream may still read the old one, so
// the host waits for the stream before it goes
template <class T> int reserve_idle(uvaia_clust_ctx *c, DevBuf<T> &b, size_t n)
{
  if (n <= b.cap) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return b.reserve(c, n);
}

// One timed launch: launch() between the context's two events (timed_issue), the wait for the second, the time added to `acc` (timed_take).
// The merge round queues its copy back between the two halves and waits for the stream once.
template <class F> int timed_issue(uvaia_clust_ctx *c, F launch)
{
  HIPCHK(c, hipEventRecord(c->ev_a, c->stream));
  launch();
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_b, c->stream));
  return 0;
}
int timed_take(uvaia_clust_ctx *c, double &acc)
{
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
  acc += ms;
  return 0;
}
template <class F> int timed(uvaia_clust_ctx *c, double &acc, F launch)
{
  if (int rc = timed_issue(c, launch)) return rc;
  HIPCHK(c, hipEventSynchronize(c->ev_b));
  return timed_take(c, acc);
}

int ensure_rows(uvaia_clust_ctx *c, size_t need)
{
  if (need <= c->rows_cap) return 0;
  const size_t cap = std::max(need, std::max<size_t>(c->rows_cap * 2, 1024));
  const size_t old = (size_t)c->pushed, np = (size_t)std::max(c->n_score, 1);
  int rc;
  if (c->keep) {                       // the text of the rows is not kept: their slots are
    if ((rc = c->d_slot.grow_keeping(c, cap, old, c->stream))) return rc;
  } else {
    c->peak_row_bytes = std::max(c->peak_row_bytes, (c->rows_cap + cap) * c->pitch);     // grow_keeping holds the old and the new array at once
    if ((rc = c->d_rows.grow_keeping(c, cap * c->pitch, old * c->pitch, c->stream))) return rc;
  }
  if ((rc = c->d_dist.grow_keeping(c, cap, old, c->stream))) return rc;
  if ((rc = c->d_p.grow_keeping(c, cap * np, old * np, c->stream))) return rc;
  if ((rc = c->d_join.grow_keeping(c, cap, old, c->stream))) return rc;
  c->rows_cap = cap;
  return 0;
}

// medoid slots per queue: at least as many as rows pushed to the busiest queue.  A queue's row of m_ord, m_st and m_loc moves from m_cap to
// cap ints apart; the new arrays join the context only once all of them exist and hold the old entries.
int ensure_medoids(uvaia_clust_ctx *c, long long need)
{
  if (need <= c->m_cap) return 0;
  if (need > INT_MAX / 2) return cfail(c, UVAIA_GPU_EINVAL, "more than %d sequences in one queue", INT_MAX / 2);
  const int cap = (int)std::max<long long>(need, std::max(2LL * c->m_cap, 256LL));
  DevBuf<int> *const held[3] = {&c->d_mord, &c->d_mst, &c->d_mloc};
  DevBuf<int> made[3];
  for (int k = 0; k < (c->keep ? 3 : 2); k++) {
    if (int rc = made[k].reserve(c, (size_t)c->n_queues * cap)) return rc;
    if (c->m_cap) HIPCHK(c, hipMemcpy2DAsync(made[k].p, (size_t)cap * sizeof(int), held[k]->p, (size_t)c->m_cap * sizeof(int), (size_t)c->m_cap * sizeof(int), c->n_queues, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; k++) *held[k] = std::move(made[k]);
  c->m_cap = cap;
  return 0;
}

struct uvdb_like_exc { uint32_t pos, len_char; };   // an exception record as a packed database file holds it (host/uvdb.h)

size_t row_bytes_now(const uvaia_clust_ctx *c)
{
  return c->keep ? c->slabs.size() * (size_t)c->slab_rows * c->pitch + c->d_stage.cap : c->rows_cap * c->pitch;
}

// keep medoids: slabs for `need` slots.  A new slab is a new allocation: nothing is copied, the table of base pointers is sent again.
int ensure_slabs(uvaia_clust_ctx *c, long long need)
{
  const size_t want = (size_t)((need + c->slab_rows - 1) >> c->slab_shift);
  if (want <= c->slabs.size()) return 0;
  while (c->slabs.size() < want) {
    DevBuf<uint8_t> slab;
    if (int rc = slab.reserve(c, (size_t)c->slab_rows * c->pitch)) return rc;
    c->slabs.push_back(std::move(slab));
  }
  if (want > c->d_slabtab.cap) if (int rc = reserve_idle(c, c->d_slabtab, std::max(want, 2 * c->d_slabtab.cap))) return rc;
  std::vector<uint8_t *> tab(c->slabs.begin(), c->slabs.end());
  HIPCHK(c, hipMemcpyAsync(c->d_slabtab, tab.data(), tab.size() * sizeof(uint8_t *), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->peak_row_bytes = std::max(c->peak_row_bytes, row_bytes_now(c));
  return 0;
}

// where the n rows of a push (ordinals first ..) are written: their place in the store, or the staging buffer
int push_rows_dst(uvaia_clust_ctx *c, long long first, int n, uint8_t **dst)
{
  int rc;
  if ((rc = ensure_rows(c, (size_t)first + n))) return rc;
  if (c->keep) {
    if ((rc = reserve_idle(c, c->d_stage, (size_t)n * c->pitch))) return rc;
    *dst = c->d_stage;
  } else *dst = c->d_rows + (size_t)first * c->pitch;
  c->peak_row_bytes = std::max(c->peak_row_bytes, row_bytes_now(c));
  return 0;
}

SlabRows slab_rows_of(const uvaia_clust_ctx *c, long long first)
{
  return SlabRows{c->d_stage, c->d_slabtab, c->pitch, c->d_slot, c->d_mloc, first, c->slab_shift, c->slab_rows - 1};
}

// the row addressing of the context's residency mode, handed to f (a generic callable: the kernels take it as a template parameter);
// first: the push ordinal of the first row in staging
template <class F> void with_rows(const uvaia_clust_ctx *c, long long first, F f)
{
  if (c->keep) f(slab_rows_of(c, first)); else f(FlatRows{c->d_rows, c->pitch});
}

// what both kinds of push check first
int push_check(uvaia_clust_ctx *c, int n, bool have_data, const int *queue)
{
  if (int rc = usable(c)) return rc;
  if (c->finished) return cfail(c, UVAIA_GPU_ESTATE, "push after finish");
  if (n < 0 || (n && (!have_data || !queue))) return cfail(c, UVAIA_GPU_EINVAL, "bad push arguments");
  if (c->pushed + n > INT_MAX / 2) return cfail(c, UVAIA_GPU_EINVAL, "more than %d sequences", INT_MAX / 2);
  for (int i = 0; i < n; i++)
    if (queue[i] < 0 || queue[i] >= c->n_queues) return cfail(c, UVAIA_GPU_EINVAL, "sequence %d of the push: queue %d out of range [0, %d)", i, queue[i], c->n_queues);
  return 0;
}

// per-queue lists of the push's ordinals (first .. first + n), in push order, and room for the medoids they may found
int push_lists(uvaia_clust_ctx *c, long long first, int n, const int *queue)
{
  const int big = INT_MAX;
  HIPCHK(c, hipMemcpyAsync(c->d_bad, &big, sizeof(int), hipMemcpyHostToDevice, c->stream));
  std::vector<int> qoff((size_t)c->n_queues + 1, 0), qlist((size_t)n);
  for (int i = 0; i < n; i++) qoff[(size_t)queue[i] + 1]++;
  for (int q = 0; q < c->n_queues; q++) qoff[(size_t)q + 1] += qoff[(size_t)q];
  { std::vector<int> fill(qoff.begin(), qoff.end() - 1); for (int i = 0; i < n; i++) qlist[(size_t)fill[(size_t)queue[i]]++] = (int)(first + i); }
  long long busiest = 0;
  for (int i = 0; i < n; i++) busiest = std::max(busiest, ++c->per_queue[(size_t)queue[i]]);
  c->queue_of.insert(c->queue_of.end(), queue, queue + n);
  int rc;
  if ((rc = ensure_medoids(c, busiest))) return rc;
  if ((rc = c->d_qlist.reserve(c, (size_t)n))) return rc;   // (no wait: its one reader, the queue kernel of the push before, was waited for by that push)
  HIPCHK(c, hipMemcpyAsync(c->d_qoff, qoff.data(), qoff.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_qlist, qlist.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (c->keep) {
    if ((rc = reserve_idle(c, c->d_pq, (size_t)n))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_pq, queue, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));            // qoff and qlist leave scope
  return 0;
}

// keep medoids, after the queue kernel: slots for the founders of the push, their rows from staging into the slabs
int keep_founders(uvaia_clust_ctx *c, long long first, int n)
{
  const int nb = (n + KTPB - 1) / KTPB;
  int rc, founders = 0;
  if ((rc = reserve_idle(c, c->d_blk, (size_t)nb + 1))) return rc;
  hipLaunchKernelGGL(clust_founder_count_kernel, dim3((unsigned)nb), dim3(KTPB), 0, c->stream, c->d_join, first, n, c->d_blk);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(clust_founder_offsets_kernel, dim3(1), dim3(KTPB), 0, c->stream, c->d_blk, nb);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&founders, c->d_blk + nb, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (founders < 0 || founders > n) { c->broken = true; return cfail(c, UVAIA_GPU_EHIP, "push of %d sequences: %d founders counted", n, founders); }
  if ((rc = ensure_slabs(c, c->kept + founders))) return rc;          // before anything is written to a slot
  hipLaunchKernelGGL(clust_founder_slots_kernel, dim3((unsigned)nb), dim3(KTPB), 0, c->stream, c->d_join, c->d_pq, first, n, c->d_blk, (int)c->kept, c->d_slot,
                     c->d_mloc, c->m_cap);
  HIPCHK(c, hipGetLastError());
  if (founders) {
    hipLaunchKernelGGL(clust_keep_founders_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, c->d_stage, c->pitch, first, c->d_slot, c->d_slabtab, c->slab_shift,
                       c->slab_rows - 1);
    HIPCHK(c, hipGetLastError());
  }
  c->h_slot.resize((size_t)first + n);
  HIPCHK(c, hipMemcpyAsync(c->h_slot.data() + first, c->d_slot + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->kept += founders;
  return 0;
}

// prep and phase 2 for the rows first .. first + n, which lie at rows (their place in the store, or staging); seq (nullable): their text on
// the host, for the message about a bad byte
int push_kernels(uvaia_clust_ctx *c, uint8_t *rows, long long first, int n, const char *const *seq)
{
  const int big = INT_MAX;
  int rc;
  // prep addresses row o at base + o * pitch: for staging the base is the address its row `first` would have, and only rows first .. are touched
  uint8_t *prep_base = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(rows) - (uintptr_t)((size_t)first * c->pitch));
  if ((rc = timed(c, c->prep_ms, [&] {
        hipLaunchKernelGGL(clust_prep_kernel, dim3((unsigned)((n + PTPB / 64 - 1) / (PTPB / 64))), dim3(PTPB), 0, c->stream, prep_base, c->pitch, first, n, c->d_ref,
                           c->nchar, c->trim, c->n_score, c->d_dist, c->d_p, c->d_bad);
      }))) return rc;
  int bad = big;
  HIPCHK(c, hipMemcpy(&bad, c->d_bad, sizeof(int), hipMemcpyDeviceToHost));
  if (bad != big) {
    c->broken = true;
    for (int k = 0; seq && k < c->nchar; k++) {
      const unsigned char b = (unsigned char)seq[bad][k];
      if (b == 0 || b >= 0x80) return cfail(c, UVAIA_GPU_EALPHABET, "sequence %lld (push ordinal) holds byte 0x%02x at site %d: only bytes 1-127 are defined", first + bad, b, k);
    }
    return cfail(c, UVAIA_GPU_EALPHABET, "sequence %lld (push ordinal) holds a byte 0 or >= 0x80", first + bad);
  }
  if ((rc = timed(c, c->queue_ms, [&] {
        with_rows(c, first, [&](auto rows_at) {
          hipLaunchKernelGGL(clust_queue_kernel<decltype(rows_at)>, dim3((unsigned)c->n_queues), dim3(QTPB), 0, c->stream, rows_at, c->nchar, c->trim, c->dist, c->n_score,
                             c->d_dist, c->d_p, c->d_qoff, c->d_qlist, c->d_mcount, c->d_mord, c->d_mst, c->m_cap, c->d_join);
        });
      }))) return rc;
  if (c->keep) if ((rc = keep_founders(c, first, n))) return rc;
  c->pushed += n;
  return 0;
}

// rows ordinal[0 .. n) into the gather buffer, row k at d_gather + k * pitch.  Keep medoids: every ordinal must have founded a cluster.
int gather_rows(uvaia_clust_ctx *c, const int64_t *ordinal, int n)
{
  std::vector<int> ord((size_t)n);
  for (int k = 0; k < n; k++) {
    if (ordinal[k] < 0 || ordinal[k] >= c->pushed) return cfail(c, UVAIA_GPU_EINVAL, "ordinal[%d] = %lld: %lld sequences were pushed", k, (long long)ordinal[k], c->pushed);
    if (c->keep && c->h_slot[(size_t)ordinal[k]] < 0)
      return cfail(c, UVAIA_GPU_EINVAL, "ordinal[%d] = %lld joined a cluster: this context keeps the rows of the sequences that founded one only", k, (long long)ordinal[k]);
    ord[(size_t)k] = (int)ordinal[k];
  }
  hipSetDevice(c->device);
  int rc;
  if ((rc = reserve_idle(c, c->d_gord, (size_t)n))) return rc;
  if ((rc = reserve_idle(c, c->d_gather, (size_t)n * c->pitch))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_gord, ord.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  with_rows(c, c->pushed, [&](auto rows_at) {
    hipLaunchKernelGGL(clust_gather_rows_kernel<decltype(rows_at)>, dim3((unsigned)n), dim3(256), 0, c->stream, rows_at, c->d_gord, c->d_gather);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));        // ord leaves scope
  return 0;
}

struct Clust {
  int ord;                          // push ordinal of the medoid
  int stored;                       // score[0] as the reference leaves it
  std::vector<long long> members;   // the nn list
};

// compare_fastaseq_score (src/fastaseq.c:31-40): score vectors descending; true when a goes strictly before b
struct ScoreOrder {
  const std::vector<int> *p; int n_score, nchar;
  int key(const Clust &x, int i) const { return i == 0 ? x.stored : (i <= n_score ? (*p)[(size_t)x.ord * n_score + i - 1] : nchar); }
  bool operator()(const Clust &a, const Clust &b) const
  {
    for (int i = 0; i < n_score + 2; i++) { const int ka = key(a, i), kb = key(b, i); if (ka != kb) return ka > kb; }
    return false;
  }
};

// ---- uvaia_clust_finish, step by step.  L[q]: the cluster list queue q holds now.

// the queues' medoid lists as phase 2 left them, the members attached; p: the score positions of every row
int read_lists(uvaia_clust_ctx *c, std::vector<std::vector<Clust>> &L, std::vector<int> &p)
{
  const int Q = c->n_queues, ns = c->n_score;
  const size_t N = (size_t)c->pushed;
  std::vector<int> mcount((size_t)Q), join(N), mord((size_t)Q * c->m_cap), mst((size_t)Q * c->m_cap);
  p.resize(N * (size_t)ns);
  HIPCHK(c, hipMemcpy(mcount.data(), c->d_mcount, (size_t)Q * sizeof(int), hipMemcpyDeviceToHost));
  if (N) HIPCHK(c, hipMemcpy(join.data(), c->d_join, N * sizeof(int), hipMemcpyDeviceToHost));
  if (N && ns) HIPCHK(c, hipMemcpy(p.data(), c->d_p, N * ns * sizeof(int), hipMemcpyDeviceToHost));
  if (c->m_cap) {
    HIPCHK(c, hipMemcpy(mord.data(), c->d_mord, mord.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(mst.data(), c->d_mst, mst.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  L.assign((size_t)Q, {});
  for (int q = 0; q < Q; q++) {
    L[(size_t)q].resize((size_t)mcount[(size_t)q]);
    for (int s = 0; s < mcount[(size_t)q]; s++) {
      Clust &k = L[(size_t)q][(size_t)s];
      k.ord = mord[(size_t)q * c->m_cap + s]; k.stored = mst[(size_t)q * c->m_cap + s];
    }
  }
  // members in push order, which is queue order: join[o] is a slot of o's own queue
  for (size_t o = 0; o < N; o++) if (join[o] >= 0) L[(size_t)c->queue_of[o]][(size_t)join[o]].members.push_back((long long)o);
  return 0;
}

// One round of the merge tree over cc lists: list j absorbs list j + cc / 2 + cc % 2.  An item is an absorbed cluster with its window
// [lo, hi) of `list`, the absorbing lists laid end to end; target: the entry of `list` it joins, or -1.
struct MergeRound {
  int cc;
  std::vector<int> item_ord, item_lo, item_hi, list, target;
  std::vector<int> pair_item0, pair_list0;     // per pair: its first item, the start of its absorbing list
  int absorbed(int j) const { return j + cc / 2 + cc % 2; }
};
struct MergeBufs { DevBuf<int> item_ord, item_lo, item_hi, list, target; };

MergeRound build_round(const uvaia_clust_ctx *c, std::vector<std::vector<Clust>> &L, int cc, const ScoreOrder &by_score)
{
  MergeRound r; r.cc = cc;
  for (int j = 0; j < cc / 2; j++) {
    std::vector<Clust> &A = L[(size_t)j], &B = L[(size_t)r.absorbed(j)];
    r.pair_item0.push_back((int)r.item_ord.size()); r.pair_list0.push_back((int)r.list.size());
    if (B.empty()) continue;                                  // an empty absorbed queue: no-op
    std::stable_sort(A.begin(), A.end(), by_score);
    std::stable_sort(B.begin(), B.end(), by_score);
    if (A.empty()) continue;                                  // spliced below: A takes B as it is sorted
    const int base = (int)r.list.size();
    for (const Clust &k : A) r.list.push_back(k.ord);
    for (const Clust &k : B) {
      // A is sorted by stored distance descending: the ring |stored - k.stored| <= d is one window
      auto lo = std::partition_point(A.begin(), A.end(), [&](const Clust &x) { return x.stored > k.stored + c->dist; });
      auto hi = std::partition_point(lo, A.end(), [&](const Clust &x) { return x.stored >= k.stored - c->dist; });
      r.item_ord.push_back(k.ord); r.item_lo.push_back(base + (int)(lo - A.begin())); r.item_hi.push_back(base + (int)(hi - A.begin()));
    }
  }
  r.target.assign(r.item_ord.size(), -1);
  return r;
}

// the round on the device: items and lists up, one wave per item, the targets back; one wait for the stream
int run_round(uvaia_clust_ctx *c, MergeRound &r, MergeBufs &d)
{
  const int n_items = (int)r.item_ord.size();
  if (!n_items) return 0;
  int rc;
  // (no wait before these grow: the round before ended with a wait for the stream)
  for (DevBuf<int> *b : {&d.item_ord, &d.item_lo, &d.item_hi, &d.target}) if ((rc = b->reserve(c, (size_t)n_items))) return rc;
  if ((rc = d.list.reserve(c, r.list.size()))) return rc;
  auto up = [&](int *dst, const std::vector<int> &v) { return hipMemcpyAsync(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, c->stream); };
  HIPCHK(c, up(d.item_ord, r.item_ord)); HIPCHK(c, up(d.item_lo, r.item_lo)); HIPCHK(c, up(d.item_hi, r.item_hi)); HIPCHK(c, up(d.list, r.list));
  if ((rc = timed_issue(c, [&] {
        with_rows(c, c->pushed, [&](auto rows_at) {
          hipLaunchKernelGGL(clust_merge_kernel<decltype(rows_at)>, dim3((unsigned)((n_items + PTPB / 64 - 1) / (PTPB / 64))), dim3(PTPB), 0, c->stream, rows_at, c->nchar,
                             c->trim, c->dist, d.item_ord, d.item_lo, d.item_hi, d.list, n_items, d.target);
        });
      }))) return rc;
  HIPCHK(c, hipMemcpyAsync(r.target.data(), d.target, (size_t)n_items * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return timed_take(c, c->merge_ms);
}

// splice, in the absorbed list's sorted order (src/fastaseq.c:228-253)
void splice_round(std::vector<std::vector<Clust>> &L, const MergeRound &r)
{
  for (int j = 0; j < r.cc / 2; j++) {
    std::vector<Clust> &A = L[(size_t)j], &B = L[(size_t)r.absorbed(j)];
    if (B.empty()) continue;
    if (A.empty()) { A.swap(B); continue; }
    int it = r.pair_item0[(size_t)j];
    const int base = r.pair_list0[(size_t)j];
    for (Clust &k : B) {
      const int t = r.target[(size_t)it++];
      if (t >= 0) {
        Clust &to = A[(size_t)(t - base)];
        to.members.push_back(k.ord);
        to.members.insert(to.members.end(), k.members.begin(), k.members.end());
      } else A.push_back(std::move(k));
    }
    B.clear();
  }
}

// final order (src/cluster.c:233, compare_fastaseq src/fastaseq.c:23-29): more members first, then the score vectors; the result arrays
void emit_result(uvaia_clust_ctx *c, std::vector<Clust> &F, const ScoreOrder &by_score)
{
  std::stable_sort(F.begin(), F.end(), [&](const Clust &a, const Clust &b) {
    if (a.members.size() != b.members.size()) return a.members.size() > b.members.size();
    return by_score(a, b);
  });
  c->r_medoid.clear(); c->r_offsets.assign(1, 0); c->r_members.clear(); c->r_scores.clear();
  for (const Clust &k : F) {
    c->r_medoid.push_back(k.ord);
    c->r_members.insert(c->r_members.end(), k.members.begin(), k.members.end());
    c->r_offsets.push_back((long long)c->r_members.size());
    for (int s = 0; s < c->n_score + 2; s++) c->r_scores.push_back(by_score.key(k, s));
  }
}

struct CloseClust { void operator()(uvaia_clust_ctx *c) const { uvaia_clust_close(c); } };

}  // namespace

extern "C" {

const char *uvaia_clust_last_error(const uvaia_clust_ctx *c) { return c ? c->err.c_str() : g_open_error.c_str(); }

void uvaia_clust_close(uvaia_clust_ctx *c)
{
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  delete c;
}

int uvaia_clust_open(uvaia_clust_ctx **out, int device, const char *reference, int nchar, int dist, int trim, int n_score, int n_queues)
{
  if (!out) return cfail(nullptr, UVAIA_GPU_EINVAL, "null output pointer");
  *out = nullptr;
  if (!reference || nchar < 1) return cfail(nullptr, UVAIA_GPU_EINVAL, "empty reference sequence");
  if (dist < 0 || trim < 0 || n_score < 0 || n_queues < 1 || 2LL * trim >= nchar)
    return cfail(nullptr, UVAIA_GPU_EINVAL, "bad parameters: distance %d, trim %d (2 trim must stay below the %d sites), n_score %d, queues %d", dist, trim, nchar, n_score, n_queues);
  for (int i = 0; i < nchar; i++) {
    const unsigned char b = (unsigned char)reference[i];
    if (b == 0 || b >= 0x80) return cfail(nullptr, UVAIA_GPU_EALPHABET, "reference site %d holds byte 0x%02x", i, b);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return cfail(nullptr, UVAIA_GPU_ENODEV, "no HIP device: clustering runs on an MI355X (gfx950) and has no CPU path");
  if (device < 0 || device >= ndev) return cfail(nullptr, UVAIA_GPU_EINVAL, "device %d out of range (%d devices)", device, ndev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return cfail(nullptr, UVAIA_GPU_ENODEV, "cannot query device %d", device);
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return cfail(nullptr, UVAIA_GPU_ENODEV, "device %d is %s: this library is built for gfx950 only", device, prop.gcnArchName);
  if (hipSetDevice(device) != hipSuccess) return cfail(nullptr, UVAIA_GPU_ENODEV, "cannot select device %d", device);
  std::unique_ptr<uvaia_clust_ctx, CloseClust> c(new uvaia_clust_ctx());   // a failure below closes the half-made context; its message goes to uvaia_clust_last_error(NULL)
  c->device = device; c->nchar = nchar; c->dist = dist; c->trim = trim; c->n_score = n_score; c->n_queues = n_queues;
  c->pitch = ((size_t)nchar + 63) & ~(size_t)63;
  c->per_queue.assign((size_t)n_queues, 0);
  std::vector<uint8_t> ref(c->pitch, 0);
  for (int i = 0; i < nchar; i++) { const uint8_t b = (uint8_t)reference[i]; ref[(size_t)i] = (b >= 'a' && b <= 'z') ? b - 32 : b; }
  int rc;
  HIPCHK(nullptr, hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
  if ((rc = c->ev_a.make(nullptr)) || (rc = c->ev_b.make(nullptr))) return rc;
  if ((rc = c->d_ref.reserve(nullptr, c->pitch))) return rc;
  HIPCHK(nullptr, hipMemcpy(c->d_ref, ref.data(), c->pitch, hipMemcpyHostToDevice));
  if ((rc = c->d_bad.reserve(nullptr, 1)) || (rc = c->d_qoff.reserve(nullptr, (size_t)n_queues + 1)) || (rc = c->d_mcount.reserve(nullptr, (size_t)n_queues))) return rc;
  HIPCHK(nullptr, hipMemset(c->d_mcount, 0, (size_t)n_queues * sizeof(int)));
  *out = c.release();
  return 0;
}

int uvaia_clust_push(uvaia_clust_ctx *c, int n, const char *const *seq, const int *queue)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = push_check(c, n, seq != nullptr, queue)) return rc;
  if (!n) return 0;
  for (int i = 0; i < n; i++) if (!seq[i]) return cfail(c, UVAIA_GPU_EINVAL, "sequence %d of the push is null", i);
  hipSetDevice(c->device);
  int rc;
  const long long first = c->pushed;
  uint8_t *dst = nullptr;
  if ((rc = push_rows_dst(c, first, n, &dst))) return rc;
  // rows, padded with zero bytes to the pitch
  c->h_rows.assign((size_t)n * c->pitch, 0);
  for (int i = 0; i < n; i++) memcpy(c->h_rows.data() + (size_t)i * c->pitch, seq[i], (size_t)c->nchar);
  HIPCHK(c, hipMemcpyAsync(dst, c->h_rows.data(), c->h_rows.size(), hipMemcpyHostToDevice, c->stream));
  if ((rc = push_lists(c, first, n, queue))) return rc;
  return push_kernels(c, dst, first, n, seq);
}

int uvaia_clust_push_packed(uvaia_clust_ctx *c, int n, const void *planes, const uint64_t *exc_offsets, const void *exc, const int *queue)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = push_check(c, n, planes != nullptr, queue)) return rc;
  if (!n) return 0;
  // the exception records, from the caller's arrays (a file mapping) as they are about to be copied: nothing of a bad record reaches the device
  const uvdb_like_exc *rec = reinterpret_cast<const uvdb_like_exc *>(exc);
  const uint64_t x0 = exc_offsets ? exc_offsets[0] : 0, x1 = exc_offsets ? exc_offsets[n] : 0;
  if (exc_offsets) {
    for (int i = 0; i < n; i++) if (exc_offsets[i + 1] < exc_offsets[i]) return cfail(c, UVAIA_GPU_EINVAL, "exc_offsets[%d] decreases", i + 1);
    if (x1 - x0 > (uint64_t)INT_MAX) return cfail(c, UVAIA_GPU_EINVAL, "%llu exception records in one push", (unsigned long long)(x1 - x0));
    if (x1 > x0 && !rec) return cfail(c, UVAIA_GPU_EINVAL, "null exception records");
    for (int i = 0; i < n; i++) {
      uint64_t at = 0;                                 // end of the row's previous run
      for (uint64_t e = exc_offsets[i]; e < exc_offsets[i + 1]; e++) {
        const uint64_t pos = rec[e].pos, len = rec[e].len_char >> 8;
        const unsigned ch = rec[e].len_char & 0xffu;
        if (ch != '-' && ch != '?' && ch != 'X' && ch != 'O' && ch != '.')
          return cfail(c, UVAIA_GPU_EINVAL, "sequence %d of the push: exception record %llu holds character 0x%02x (only - ? X O . are exceptions)", i, (unsigned long long)(e - exc_offsets[i]), ch);
        if (pos + len > (uint64_t)c->nchar)
          return cfail(c, UVAIA_GPU_EINVAL, "sequence %d of the push: exception run of %llu sites at site %llu ends beyond the %d sites of a row", i, (unsigned long long)len, (unsigned long long)pos, c->nchar);
        if (pos < at) return cfail(c, UVAIA_GPU_EINVAL, "sequence %d of the push: exception runs overlap or are out of order at site %llu", i, (unsigned long long)pos);
        at = pos + len;
      }
    }
  }
  hipSetDevice(c->device);
  int rc;
  const long long first = c->pushed;
  uint8_t *dst = nullptr;
  if ((rc = push_rows_dst(c, first, n, &dst))) return rc;
  const int W4 = ((c->nchar + 31) / 32 + 3) / 4, n_tiles = (n + 63) / 64;
  const size_t tile_bytes = (size_t)W4 * 4 * 64 * 16, n_rec = (size_t)(x1 - x0);
  if ((rc = reserve_idle(c, c->d_tiles, (size_t)n_tiles * tile_bytes))) return rc;
  if ((rc = reserve_idle(c, c->d_xoff, (size_t)n + 1))) return rc;
  if (n_rec && (rc = reserve_idle(c, c->d_xrec, n_rec))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_tiles, planes, (size_t)n_tiles * tile_bytes, hipMemcpyHostToDevice, c->stream));
  if (n_rec) {
    c->h_xoff.resize((size_t)n + 1);
    for (int i = 0; i <= n; i++) c->h_xoff[(size_t)i] = (uint32_t)(exc_offsets[i] - x0);
    HIPCHK(c, hipMemcpyAsync(c->d_xoff, c->h_xoff.data(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_xrec, rec + x0, n_rec * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
  }
  const int units = (W4 + UGROUPS - 1) / UGROUPS;
  if ((rc = timed(c, c->decode_ms, [&] {
        hipLaunchKernelGGL(clust_unpack_tiles_kernel, dim3((unsigned)(n_tiles * units)), dim3(UTPB), 0, c->stream, reinterpret_cast<const uint4 *>(c->d_tiles.p), W4, c->nchar, n,
                           dst, c->pitch, units);
      }))) return rc;
  if (n_rec && (rc = timed(c, c->overlay_ms, [&] {
        hipLaunchKernelGGL(clust_overlay_runs_kernel, dim3((unsigned)n), dim3(OTPB), 0, c->stream, dst, c->pitch, c->d_xoff, c->d_xrec);
      }))) return rc;
  if ((rc = push_lists(c, first, n, queue))) return rc;
  return push_kernels(c, dst, first, n, nullptr);
}

int uvaia_clust_push_device(uvaia_clust_ctx *c, int n, const void *d_rows, size_t pitch, const int *row_index, const int *queue)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = push_check(c, n, d_rows != nullptr, queue)) return rc;
  if (!n) return 0;
  // the block, before anything is launched: the largest row the selection names must lie inside the allocation the pointer belongs to
  long long last = row_index ? -1 : (long long)n - 1;
  for (int i = 0; row_index && i < n; i++) {
    if (row_index[i] < 0) return cfail(c, UVAIA_GPU_EINVAL, "row_index[%d] = %d is negative", i, row_index[i]);
    last = std::max<long long>(last, row_index[i]);
  }
  hipSetDevice(c->device);
  char msg[256];
  if (!rows_block_ok(d_rows, pitch, c->nchar, c->device, last, msg, sizeof msg)) return cfail(c, UVAIA_GPU_EINVAL, "%s", msg);
  int rc;
  const long long first = c->pushed;
  uint8_t *dst = nullptr;
  if ((rc = push_rows_dst(c, first, n, &dst))) return rc;
  if (row_index) {
    if ((rc = reserve_idle(c, c->d_rsel, (size_t)n))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_rsel, row_index, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = timed(c, c->rows_in_ms, [&] {
        hipLaunchKernelGGL(clust_rows_in_kernel, dim3((unsigned)n), dim3(RTPB), 0, c->stream, reinterpret_cast<const uint8_t *>(d_rows), pitch, c->nchar,
                           row_index ? c->d_rsel.p : (const int *)nullptr, dst, c->pitch);
      }))) return rc;                                  // (the caller's rows have been read: it may overwrite them)
  if ((rc = push_lists(c, first, n, queue))) return rc;
  return push_kernels(c, dst, first, n, nullptr);
}

int uvaia_clust_push_device_ms(uvaia_clust_ctx *c, double *rows_in_ms)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (rows_in_ms) *rows_in_ms = c->rows_in_ms;
  return 0;
}

int uvaia_clust_rows(uvaia_clust_ctx *c, const int64_t *ordinal, int n, char *rows, size_t pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = usable(c)) return rc;
  if (n < 0 || (n && (!ordinal || !rows))) return cfail(c, UVAIA_GPU_EINVAL, "bad arguments");
  if (n && pitch < (size_t)c->nchar) return cfail(c, UVAIA_GPU_EINVAL, "pitch %zu is below the %d sites of a row", pitch, c->nchar);
  if (!n) return 0;
  if (int rc = gather_rows(c, ordinal, n)) return rc;
  HIPCHK(c, hipMemcpy2DAsync(rows, pitch, c->d_gather, c->pitch, (size_t)c->nchar, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int uvaia_clust_gather_device(uvaia_clust_ctx *c, const int64_t *ordinal, int n, const void **d_rows, size_t *pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = usable(c)) return rc;
  if (n < 0 || (n && !ordinal)) return cfail(c, UVAIA_GPU_EINVAL, "bad arguments");
  if (n) {
    if (int rc = gather_rows(c, ordinal, n)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (d_rows) *d_rows = n ? c->d_gather.p : nullptr;
  if (pitch) *pitch = c->pitch;
  return 0;
}

int uvaia_clust_device_rows(uvaia_clust_ctx *c, const void **d_rows, size_t *pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = usable(c)) return rc;
  if (c->keep) return cfail(c, UVAIA_GPU_ESTATE, "this context keeps medoid rows only, in slabs: there is no row store to hand out; uvaia_clust_gather_device gives the rows of medoids");
  if (d_rows) *d_rows = c->d_rows;
  if (pitch) *pitch = c->pitch;
  return 0;
}

int uvaia_clust_keep_medoids(uvaia_clust_ctx *c, int slab_rows)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = usable(c)) return rc;
  if (c->pushed || c->finished) return cfail(c, UVAIA_GPU_ESTATE, "uvaia_clust_keep_medoids after a push: the mode is chosen before the first one");
  if (slab_rows < 0 || (slab_rows & (slab_rows - 1))) return cfail(c, UVAIA_GPU_EINVAL, "slab_rows %d is not a power of two", slab_rows);
  c->keep = true;
  c->slab_rows = slab_rows ? slab_rows : SLAB_ROWS;
  c->slab_shift = 0;
  while ((1 << c->slab_shift) < c->slab_rows) c->slab_shift++;
  return 0;
}

int uvaia_clust_memory(uvaia_clust_ctx *c, size_t *row_bytes, size_t *peak_row_bytes, size_t *free_bytes)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (row_bytes) *row_bytes = row_bytes_now(c);
  if (peak_row_bytes) *peak_row_bytes = std::max(c->peak_row_bytes, row_bytes_now(c));
  if (free_bytes) {
    size_t fr = 0, total = 0;
    hipSetDevice(c->device);
    if (hipMemGetInfo(&fr, &total) != hipSuccess) return cfail(c, UVAIA_GPU_EHIP, "cannot query the free memory of device %d", c->device);
    *free_bytes = fr;
  }
  return 0;
}

int uvaia_clust_finish(uvaia_clust_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = usable(c)) return rc;
  if (c->finished) return cfail(c, UVAIA_GPU_ESTATE, "finish called twice");
  hipSetDevice(c->device);
  std::vector<std::vector<Clust>> L;
  std::vector<int> p;
  if (int rc = read_lists(c, L, p)) return rc;
  const ScoreOrder by_score{&p, c->n_score, c->nchar};
  MergeBufs bufs;
  for (int cc = c->n_queues; cc > 1; cc = cc / 2 + cc % 2) {
    MergeRound r = build_round(c, L, cc, by_score);
    if (int rc = run_round(c, r, bufs)) return rc;
    splice_round(L, r);
  }
  emit_result(c, L[0], by_score);
  c->finished = true;
  return 0;
}

int uvaia_clust_result(uvaia_clust_ctx *c, int *n_clusters, int64_t *medoid, int64_t *offsets, int64_t *members, int *scores)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (!c->finished) return cfail(c, UVAIA_GPU_ESTATE, "result before finish");
  const size_t nc = c->r_medoid.size();
  if (n_clusters) *n_clusters = (int)nc;
  if (medoid) for (size_t k = 0; k < nc; k++) medoid[k] = c->r_medoid[k];
  if (offsets) for (size_t k = 0; k <= nc; k++) offsets[k] = c->r_offsets[k];
  if (members) for (size_t k = 0; k < c->r_members.size(); k++) members[k] = c->r_members[k];
  if (scores) memcpy(scores, c->r_scores.data(), c->r_scores.size() * sizeof(int));
  return 0;
}

int uvaia_clust_stats(uvaia_clust_ctx *c, double *prep_ms, double *queue_ms, double *merge_ms, int64_t *pushed)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (prep_ms) *prep_ms = c->prep_ms;
  if (queue_ms) *queue_ms = c->queue_ms;
  if (merge_ms) *merge_ms = c->merge_ms;
  if (pushed) *pushed = c->pushed;
  return 0;
}

int uvaia_clust_unpack_ms(uvaia_clust_ctx *c, double *decode_ms, double *overlay_ms)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (decode_ms) *decode_ms = c->decode_ms;
  if (overlay_ms) *overlay_ms = c->overlay_ms;
  return 0;
}

}  // extern "C"
