// kernels_pairs.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): all pairs of the resident database against each other (uvaia_gpu_db_pairs, uvaia_gpu_db_pairs_within): pairs_rows_kernel builds the row-side operand records of a band of rows, pairs_snp_kernel and pairs_counts_kernel count every (row, column) pair of a rectangle, the latter also into a list of the pairs within a distance; pairs_link_snp_kernel and the link mode of pairs_counts_kernel unite the pairs within a distance in a union-find forest instead (uvaia_gpu_db_link), pairs_labels_kernel reads the cluster labels off it; pairs_near_snp_kernel and the near mode of pairs_counts_kernel keep every reference's closest reference of another component instead (uvaia_gpu_db_near, uvaia_gpu_db_mst).

// ------------------------------------------------------------------------------------------------------------
// device: all-pairs counters over the resident four-plane tiles
// ------------------------------------------------------------------------------------------------------------
// Counters of a pair (a, b) over the sites [trim, nchar - trim), nothing truncated (include/uvaia_gpu.h):
//   0 ACGT_matches  1 text_matches  2 partial_matches  3 valid_pair_comparisons  4 ACGT_pair_comparisons
// On the planes a site is valid iff some plane bit is set and ACGT iff exactly one is; two sites are equal and valid iff the four planes are
// equal and one is set; the sets intersect iff some plane has both bits set.
//
// The column side of a pair is a lane of a resident tile, read as the scans read it.  The row side is wave-uniform: a record of dwords per
// (row, word group) at an address every lane shares, so that it arrives through scalar loads and is an SGPR operand of the bit operations.
//   SNP record,    12 dwords: lo[4] hi[4] is[4]                 (the 2-bit code of import_tiles_kernel<3> and "is ACGT", words 4 w4 .. 4 w4 + 3)
//   COUNTS record, 24 dwords: (A C G T valid single) x 4 words   (the qp layout of scan_iupac_kernel)
// rec[(row - first row of the band) * W4 + w4][dwords]; the band is padded to whole blocks of 64 rows with cleared records.
constexpr int PAIRS_SNP_DW = 12, PAIRS_CNT_DW = 24;
constexpr int PAIRS_CNT_RT = 16;      // rows per wave of pairs_counts_kernel: 80 accumulators, no scratch (kernel-resource-usage)

static __device__ __forceinline__ uint32_t pairs_window_mask(int word, int lo_site, int hi_site)
{ // the bits of alignment word `word` (sites 32 word .. 32 word + 31) that lie in [lo_site, hi_site)
  const int a = max(lo_site - word * 32, 0), b = min(hi_site - word * 32, 32);
  if (a >= b) return 0u;
  const uint32_t below_b = b >= 32 ? 0xFFFFFFFFu : ((1u << b) - 1u);
  return below_b & ~((1u << a) - 1u);                  // (a < b <= 32: the shift is defined)
}

// The trim window is applied here and only here: the row-side words are cleared outside [lo_site, hi_site), the first and last word of the
// window by bit.  Where the row side is cleared every counter of the pair is 0 whatever the column holds there (q = row side, r = column side):
//   0 ACGT_matches       counts  equal & q.single              q.single = 0                                         -> 0
//   1 text_matches       counts  equal & r.valid               a cleared row side equals the column only where the column is the empty set too
//                                                              ("equal" is 1 there), and there r.valid = 0; elsewhere equal = 0  -> 0
//   2 partial_matches    counts  (A & A') | ... | (T & T')     every row plane is 0                                 -> 0
//   3 valid_pair_comp.   counts  r.valid & q.valid             q.valid = 0                                          -> 0
//   4 ACGT_pair_comp.    counts  r.single & q.single           q.single = 0                                         -> 0
//   snp pair             counts  differ & r.is & q.is          q.is = 0                                             -> 0
// The column side therefore needs no mask, and sites at and past nchar (zero in tiles this library packed, anything in tiles that were handed
// in) never count: the window ends at nchar - trim.
// One block per (64 rows of the band, 4 word groups): thread = (row, word group) reads its four plane words as the tiles hold them (a wave =
// 64 rows of one word group, contiguous where the rows share a tile), the records are turned through LDS so that a row's 4 x D dwords leave
// as one contiguous run.
template <int D>
__global__ __launch_bounds__(256) void pairs_rows_kernel(const uint4 *__restrict__ db, int W4, long long row0, int n_rows, int lo_site, int hi_site,
                                                          uint32_t *__restrict__ rec)
{
  __shared__ uint32_t turn[64 * 4 * D];
  const int lane = threadIdx.x & 63, wq = threadIdx.x >> 6;
  const int rr = blockIdx.x * 64 + lane, w4 = blockIdx.y * 4 + wq;
  uint32_t v[D];
#pragma unroll
  for (int k = 0; k < D; k++) v[k] = 0u;
  if (rr < n_rows && w4 < W4) {
    const long long r = row0 + rr;
    const uint4 *t = db + ((size_t)(r >> 6) * W4 + w4) * 4 * 64 + (r & 63);
    const uint4 pA = t[0], pC = t[64], pG = t[128], pT = t[192];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t m = pairs_window_mask(w4 * 4 + j, lo_site, hi_site);
      const uint32_t a = u4c(pA, j) & m, cc = u4c(pC, j) & m, g = u4c(pG, j) & m, tt = u4c(pT, j) & m;
      const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
      const uint32_t single = par & ~three;
      if (D == PAIRS_SNP_DW) { v[j] = (cc | tt) & single; v[4 + j] = (g | tt) & single; v[8 + j] = single; }
      else { v[j * 6 + 0] = a; v[j * 6 + 1] = cc; v[j * 6 + 2] = g; v[j * 6 + 3] = tt; v[j * 6 + 4] = a | cc | g | tt; v[j * 6 + 5] = single; }
    }
  }
#pragma unroll
  for (int k = 0; k < D; k++) turn[(lane * 4 + wq) * D + k] = v[k];
  __syncthreads();
  const int nw = min(4, W4 - (int)blockIdx.y * 4);     // word groups of this block that exist
  for (int i = threadIdx.x; i < 64 * 4 * D; i += 256) {
    const int l = i / (4 * D), o = i % (4 * D);
    if (o < nw * D) rec[((size_t)(blockIdx.x * 64 + l) * W4 + (size_t)blockIdx.y * 4) * D + o] = turn[i];
  }
}

// The snp distance (both ACGT and different = ACGT_pair_comparisons - ACGT_matches) of RT rows x 64 columns per wave: lane = column reference,
// one column tile per wave, the four waves of a block take four neighbouring column tiles against the same rows.  The column's (lo, hi, is)
// are derived in registers once per word; per row and word  x = lo ^ lo'  (v_xor),  y = x | (hi ^ hi')  (v_bitop3),  m = y & is & is'
// (v_bitop3),  acc += popcount(m)  (v_bcnt): 4 vector instructions per pair-word, the row operands SGPRs.
// Grid: block b = (row tile b % n_rtiles, column group b / n_rtiles) -- the row tile runs fastest, so the blocks resident together read the
// same few column tiles out of the caches and each others' row records.
// out[i * ld_out + (col - col0)] for rows i < n_rows of the band and columns in [col0, col0 + n_cols); nothing else is written.
template <int RT>
__global__ __launch_bounds__(256) void pairs_snp_kernel(const uint4 *__restrict__ db, int W4, const uint32_t *__restrict__ rec, int n_rows, int n_rtiles,
                                                         long long ctile0, int n_ctiles, long long col0, int n_cols, int *__restrict__ out, size_t ld_out)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x % n_rtiles, ct = (blockIdx.x / n_rtiles) * 4 + wave;
  if (ct >= n_ctiles) return;
  int acc[RT];
#pragma unroll
  for (int r = 0; r < RT; r++) acc[r] = 0;
  const uint4 *t = db + (size_t)(ctile0 + ct) * W4 * 4 * 64 + lane;
  const size_t rstride = (size_t)W4 * PAIRS_SNP_DW;
  const uint32_t *rb = rec + (size_t)rt * RT * rstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    uint32_t cL[4], cH[4], cI[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t a = u4c(pA, j), cc = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
      const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
      cI[j] = par & ~three; cL[j] = (cc | tt) & cI[j]; cH[j] = (g | tt) & cI[j];
    }
    const uint32_t *s0 = rb + (size_t)w4 * PAIRS_SNP_DW;
    QWords<PAIRS_SNP_DW> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int r = 0; r < RT; r++) {
      if (r + 1 < RT) load_qwords(nxt, s0 + (size_t)(r + 1) * rstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t x = cL[j] ^ cur.v[j];
        const uint32_t y = B3(cH[j], cur.v[4 + j], x, (TT_A ^ TT_B) | TT_C);          // codes differ
        acc[r] = bcnt_acc(B3(y, cI[j], cur.v[8 + j], TT_A & TT_B & TT_C), acc[r]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (r + 1 < RT) cur = nxt;
    }
  }
  const long long j = (ctile0 + ct) * 64 + lane - col0;
  if (j < 0 || j >= n_cols) return;
#pragma unroll
  for (int r = 0; r < RT; r++) {
    const int i = rt * RT + r;
    if (i < n_rows) out[(size_t)i * ld_out + (size_t)j] = acc[r];
  }
}

// ---- single-linkage clusters: the pairs within a distance united in a forest (uvaia_gpu_db_link_begin / _link / _link_labels)
// parent[] holds one dword per resident reference, parent[i] = i at the start.  While link kernels run, the ONLY stores to it are agent-scope
// atomic read-modify-writes (the compare-and-swap of a hook, the atomicMin of path shortening); nothing waits for another wave, no flag is
// spun on, no fence is issued.  Why that is enough on a chip whose per-XCD L2s and per-CU L1s are not coherent within a launch:
//   - every value parent[x] ever held is x itself or a SMALLER node of x's component (a hook stores lo < hi, a shortening stores an
//     ancestor, and ancestors are smaller), so a walk over stale values only ever steps to smaller nodes of the right component: it ends;
//   - a hook succeeds only through atomicCAS(&parent[hi], hi, lo), that is on a node that IS a root at that moment, whatever the walks saw;
//   - a failed CAS hands back the real parent of hi, strictly smaller than hi, and the loop goes on from (that value, lo) -- from what the
//     CAS returned, not from a reload that might be stale again: the larger of the two nodes drops with every round, so the loop ends on its own;
//   - hooks go from the larger root to the smaller, so the root of a finished component is its smallest member: the label.
// It rests on nothing but the device-wide atomicity the list kernel's atomicAdd on *n_list already rests on.  Reads are relaxed agent-scope
// atomic loads: they go past the L1, so fewer walks start from stale values (a stale walk costs time, never the answer).
static __device__ __forceinline__ uint32_t pairs_link_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static __device__ __forceinline__ uint32_t pairs_link_root(const uint32_t *parent, uint32_t x)
{ // (p > x cannot happen; it ends the walk too, so that the walk ends whatever the array holds)
  for (;;) {
    const uint32_t p = pairs_link_load(parent + x);
    if (p >= x) return x;
    x = p;
  }
}

// One lane's hits of a row tile: bit r of `hits` links database position row_first + r to `col` (row_first + r < col).  The wave's hits
// (`total`, from ballots) are added to *n_links by ONE lane with one vector atomicAdd.  The column's root is carried from hit to hit; where
// both sides already show one root nothing is stored, which keeps a dense cluster -- every lane hitting every row -- to reads.
static __device__ __forceinline__ void pairs_link_hits(uint32_t *parent, unsigned long long *n_links, uint32_t row_first, uint32_t col, uint32_t hits,
                                                       unsigned total, int lane)
{
  if (total == 0) return;
  if (lane == 0) atomicAdd(n_links, (unsigned long long)total);
  if (!hits) return;
  const uint32_t seen = pairs_link_load(parent + col);
  uint32_t rc = seen >= col ? col : pairs_link_root(parent, seen);
  while (hits) {
    const uint32_t r = (uint32_t)__ffs((int)hits) - 1u;
    hits &= hits - 1u;
    uint32_t rr = pairs_link_root(parent, row_first + r);
    while (rr != rc) {
      const uint32_t hi = max(rr, rc), lo = min(rr, rc);
      const uint32_t old = atomicCAS(parent + hi, hi, lo);
      if (old >= hi) { rc = lo; break; }               // hooked (old == hi; a larger value cannot be there)
      rr = pairs_link_root(parent, old);               // hi had been hooked by someone else: on from its real parent
      rc = pairs_link_root(parent, lo);
    }
  }
  if (rc < seen) atomicMin(parent + col, rc);          // path shortening: an ancestor, never a plain store
}

// parent[i] = i for the references resident at uvaia_gpu_db_link_begin
__global__ __launch_bounds__(256) void pairs_link_init_kernel(uint32_t *__restrict__ parent, uint32_t n)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) parent[i] = i;
}

// labels[i] = the root of i.  A launch of its own behind the last link kernel: plain loads; parent[] is not written.
__global__ __launch_bounds__(256) void pairs_labels_kernel(const uint32_t *__restrict__ parent, uint32_t n, uint32_t *__restrict__ labels)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t x = i;
  for (;;) {
    const uint32_t p = parent[x];
    if (p >= x) break;
    x = p;
  }
  labels[i] = x;
}

// The links of RT = 32 rows x 64 columns per wave under the snp metric: the loop of pairs_snp_kernel<32> -- same operand records, same grid
// order, row operands in SGPRs, 4 vector instructions per pair-word -- and with FLOOR two more, `is & is'` (v_and) and its count (v_bcnt)
// into a second accumulator per row: ACGT_pair_comparisons, the floor's "compared".  Nothing dense is written.  hit = column and row in
// range, row < col (database positions), dist <= max_dist and with FLOOR compared >= min_compared; the hits go to pairs_link_hits.
template <bool FLOOR>
__global__ __launch_bounds__(256) void pairs_link_snp_kernel(const uint4 *__restrict__ db, int W4, const uint32_t *__restrict__ rec, long long row0, int n_rows, int n_rtiles,
                                                              long long ctile0, int n_ctiles, long long col0, int n_cols, int max_dist, int min_compared,
                                                              uint32_t *parent, unsigned long long *__restrict__ n_links)
{
  constexpr int RT = 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x % n_rtiles, ct = (blockIdx.x / n_rtiles) * 4 + wave;
  if (ct >= n_ctiles) return;
  int acc[RT], cmp[FLOOR ? RT : 1];
#pragma unroll
  for (int r = 0; r < RT; r++) { acc[r] = 0; if (FLOOR) cmp[r] = 0; }
  const uint4 *t = db + (size_t)(ctile0 + ct) * W4 * 4 * 64 + lane;
  const size_t rstride = (size_t)W4 * PAIRS_SNP_DW;
  const uint32_t *rb = rec + (size_t)rt * RT * rstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    uint32_t cL[4], cH[4], cI[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t a = u4c(pA, j), cc = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
      const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
      cI[j] = par & ~three; cL[j] = (cc | tt) & cI[j]; cH[j] = (g | tt) & cI[j];
    }
    const uint32_t *s0 = rb + (size_t)w4 * PAIRS_SNP_DW;
    QWords<PAIRS_SNP_DW> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int r = 0; r < RT; r++) {
      if (r + 1 < RT) load_qwords(nxt, s0 + (size_t)(r + 1) * rstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t x = cL[j] ^ cur.v[j];
        const uint32_t y = B3(cH[j], cur.v[4 + j], x, (TT_A ^ TT_B) | TT_C);          // codes differ
        acc[r] = bcnt_acc(B3(y, cI[j], cur.v[8 + j], TT_A & TT_B & TT_C), acc[r]);
        if (FLOOR) cmp[r] = bcnt_acc(cI[j] & cur.v[8 + j], cmp[r]);                   // both ACGT
      }
      __builtin_amdgcn_sched_barrier(0);
      if (r + 1 < RT) cur = nxt;
    }
  }
  const long long col = (ctile0 + ct) * 64 + lane, j = col - col0;
  const bool col_ok = j >= 0 && j < n_cols;
  uint32_t hits = 0;                                   // bit r: this lane's column is linked to row r of the tile
  unsigned total = 0;                                  // wave-uniform: ballots
#pragma unroll
  for (int r = 0; r < RT; r++) {
    const int i = rt * RT + r;
    const bool h = col_ok && i < n_rows && row0 + i < col && acc[r] <= max_dist && (!FLOOR || cmp[r] >= min_compared);
    total += (unsigned)__popcll(__ballot(h));
    hits |= (uint32_t)h << r;
  }
  pairs_link_hits(parent, n_links, (uint32_t)(row0 + rt * RT), (uint32_t)col, hits, total, lane);
}

// ---- every reference's closest reference of another component (uvaia_gpu_db_near_* / uvaia_gpu_db_mst)
// comp[] holds one dword per resident reference, written by a copy or by pairs_near_init_kernel BEFORE the launch and only read by it: plain
// loads.  best[] holds one packed key (dist << 32 | other position) per reference, UVAIA_GPU_NEAR_NONE at the start.  While near kernels run
// the ONLY stores to best[] are agent-scope 64-bit atomicMins; nothing waits for another wave, no flag is spun on, no fence is issued.
// Why that is enough where the per-XCD L2s and per-CU L1s are not coherent within a launch:
//   - best[x] only ever decreases, and every value it holds is NONE or the key of a counting pair of x, so whatever order the atomicMins
//     of the waves, launches and calls arrive in, the cell ends as the minimum of the keys offered: a function of the rows and comp[] alone;
//   - the guard in front of an atomicMin is a relaxed agent-scope load; a stale value is one the cell held EARLIER, that is a larger one:
//     the guard then lets an atomicMin through that changes nothing.  It can never hold one back that would have lowered the cell;
//   - the host reads best[] behind the stream, after the last kernel has ended.
// Ties: the key orders by (dist, other position), and a candidate is already the smallest of its wave under that order -- the column side
// keeps the first of ascending rows by a strict <, the row side takes the lowest lane of the ballot of the wave's minimum.
constexpr uint32_t PAIRS_NEAR_NO = 0xFFFFFFFFu;        // no counting pair yet: above every distance (a distance is a number of sites)

static __device__ __forceinline__ uint32_t pairs_wave_umin(uint32_t v)
{ // the minimum over the 64 lanes, wave-uniform (every lane is active where this is called)
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, s));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

static __device__ __forceinline__ void pairs_near_lower(unsigned long long *p, unsigned long long key)
{ // (a stale, larger value costs an atomic and never the answer)
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
}

// What a wave carries from the prologue to the epilogue, and the epilogue's running minima.  RT rows x 64 columns: lane = column, lanes
// 0 .. RT - 1 also hold the row side (comp of row `lane` of the tile, and at the end that row's candidate).
template <int RT> struct PairsNear {
  uint32_t cc, rc;                                     // comp[col] of this lane; comp[row_first + lane] in lanes below RT
  uint32_t cd = PAIRS_NEAR_NO, crow = 0;               // column side: the smallest (dist, row) of this lane's column
  uint32_t rd = PAIRS_NEAR_NO, rcol = 0;               // row side, lane r: the smallest (dist, lane of the column) of row r
  long long row_first, col; int rows_here, lane; bool col_ok;

  // Prologue.  true: every row and column of the tile pair that is in range carries one comp (rows and columns out of range count as
  // "same"), so no pair of it can count and the wave returns before the loop.  Wave-uniform: ballots and a readlane.  One lane adds the
  // tile pair to stats[0] (walked) or stats[1] (skipped) by one vector atomicAdd.
  __device__ __forceinline__ bool same(const uint32_t *__restrict__ comp, unsigned long long *__restrict__ stats)
  {
    const bool row_ok = lane < RT && lane < rows_here;
    cc = col_ok ? comp[col] : 0u;
    rc = row_ok ? comp[row_first + lane] : 0u;
    const unsigned long long vc = __ballot(col_ok), vr = __ballot(row_ok);
    bool one = true;
    if (vc && vr) {
      const uint32_t ref = (uint32_t)__builtin_amdgcn_readlane((int)cc, __ffsll((long long)vc) - 1);
      one = __ballot((col_ok && cc != ref) || (row_ok && rc != ref)) == 0ull;
    }
    if (lane == 0) atomicAdd(stats + (one ? 1 : 0), 1ull);
    return one;
  }

  // Epilogue, row r of the tile (r a constant of the unrolled loop, rows ascend): a pair counts when row and column are in range,
  // row < col (database positions), the two comp differ and `floor_ok`.
  __device__ __forceinline__ void row(int r, int dist, bool floor_ok)
  {
    const uint32_t rcr = (uint32_t)__builtin_amdgcn_readlane((int)rc, r);
    const bool counts = col_ok && r < rows_here && row_first + r < col && rcr != cc && floor_ok;
    const uint32_t key = counts ? (uint32_t)dist : PAIRS_NEAR_NO;
    if (key < cd) { cd = key; crow = (uint32_t)(row_first + r); }
    const uint32_t m = pairs_wave_umin(key);
    if (m != PAIRS_NEAR_NO) {                          // (wave-uniform)
      const unsigned long long holders = __ballot(key == m);      // lanes ascend with the column: the lowest bit is the smallest column
      if (lane == r) { rd = m; rcol = (uint32_t)(__ffsll((long long)holders) - 1); }
    }
  }

  __device__ __forceinline__ void flush(unsigned long long *best)
  {
    if (cd != PAIRS_NEAR_NO) pairs_near_lower(best + col, ((unsigned long long)cd << 32) | crow);
    if (lane < RT && rd != PAIRS_NEAR_NO) pairs_near_lower(best + row_first + lane, ((unsigned long long)rd << 32) | (uint32_t)(col - lane + rcol));
  }
};

// best[i] = NONE for the references resident at uvaia_gpu_db_near_begin, and with `identity` every reference a component of its own
__global__ __launch_bounds__(256) void pairs_near_init_kernel(unsigned long long *__restrict__ best, uint32_t *__restrict__ comp, uint32_t n, int identity)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  best[i] = ~0ull;
  if (identity) comp[i] = i;
}

// Every row's and column's closest reference of another component among RT = 32 rows x 64 columns per wave under the snp metric: the loop of
// pairs_link_snp_kernel -- same operand records, same grid order, row operands in SGPRs, 4 vector instructions per pair-word, 6 with
// FLOOR -- between the prologue and the epilogue of PairsNear.  Nothing dense is written.
template <bool FLOOR>
__global__ __launch_bounds__(256) void pairs_near_snp_kernel(const uint4 *__restrict__ db, int W4, const uint32_t *__restrict__ rec, long long row0, int n_rows, int n_rtiles,
                                                              long long ctile0, int n_ctiles, long long col0, int n_cols, int min_compared,
                                                              const uint32_t *__restrict__ comp, unsigned long long *best, unsigned long long *__restrict__ stats)
{
  constexpr int RT = 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x % n_rtiles, ct = (blockIdx.x / n_rtiles) * 4 + wave;
  if (ct >= n_ctiles) return;
  PairsNear<RT> near;
  near.col = (ctile0 + ct) * 64 + lane; near.col_ok = near.col >= col0 && near.col - col0 < n_cols;
  near.row_first = row0 + (long long)rt * RT; near.rows_here = n_rows - rt * RT; near.lane = lane;
  if (near.same(comp, stats)) return;
  int acc[RT], cmp[FLOOR ? RT : 1];
#pragma unroll
  for (int r = 0; r < RT; r++) { acc[r] = 0; if (FLOOR) cmp[r] = 0; }
  const uint4 *t = db + (size_t)(ctile0 + ct) * W4 * 4 * 64 + lane;
  const size_t rstride = (size_t)W4 * PAIRS_SNP_DW;
  const uint32_t *rb = rec + (size_t)rt * RT * rstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    uint32_t cL[4], cH[4], cI[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t a = u4c(pA, j), cc = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
      const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
      cI[j] = par & ~three; cL[j] = (cc | tt) & cI[j]; cH[j] = (g | tt) & cI[j];
    }
    const uint32_t *s0 = rb + (size_t)w4 * PAIRS_SNP_DW;
    QWords<PAIRS_SNP_DW> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int r = 0; r < RT; r++) {
      if (r + 1 < RT) load_qwords(nxt, s0 + (size_t)(r + 1) * rstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t x = cL[j] ^ cur.v[j];
        const uint32_t y = B3(cH[j], cur.v[4 + j], x, (TT_A ^ TT_B) | TT_C);          // codes differ
        acc[r] = bcnt_acc(B3(y, cI[j], cur.v[8 + j], TT_A & TT_B & TT_C), acc[r]);
        if (FLOOR) cmp[r] = bcnt_acc(cI[j] & cur.v[8 + j], cmp[r]);                   // both ACGT
      }
      __builtin_amdgcn_sched_barrier(0);
      if (r + 1 < RT) cur = nxt;
    }
  }
#pragma unroll
  for (int r = 0; r < RT; r++) near.row(r, acc[r], !FLOOR || cmp[r] >= min_compared);
  near.flush(best);
}

// The five counters of PAIRS_CNT_RT rows x 64 columns per wave, same mapping and grid order as pairs_snp_kernel; the plane-equality and
// intersect chains of scan_iupac_kernel plus one `single & single'` count: 17 vector instructions per pair-word.
// MODE = PAIRS_DENSE: out[(i * ld_out + (col - col0)) * 5 + c].
// MODE = PAIRS_LIST: nothing dense is written; the pairs of the rectangle with distance <= max_dist (metric 1: count[4] - count[0], metric 2:
// count[3] - count[2]) and, with upper, row < col (database positions) go into list[]: a wave counts its hits by ballots, ONE lane reserves that
// many slots by one vector atomicAdd on *n_list, and every store is bounded by list_cap -- *n_list ends as the number of hits, whatever fitted.
// MODE = PAIRS_LINK: nothing dense and no list; the pairs row < col with distance <= max_dist and, under the same metric, compared
// (count[4] under metric 1, count[3] under metric 2) >= min_compared are united in parent[] and counted into *n_list (pairs_link_hits).
// MODE = PAIRS_NEAR: nothing dense, no list, no forest; the prologue and epilogue of PairsNear around the same loop, over that distance and
// that compared: `parent` is comp[] (only read), `n_list` the two counters of tile pairs walked and skipped, `best` the keys.
enum { PAIRS_DENSE = 0, PAIRS_LIST = 1, PAIRS_LINK = 2, PAIRS_NEAR = 3 };
template <int MODE>
__global__ __launch_bounds__(256) void pairs_counts_kernel(const uint4 *__restrict__ db, int W4, const uint32_t *__restrict__ rec, long long row0, int n_rows, int n_rtiles,
                                                            long long ctile0, int n_ctiles, long long col0, int n_cols, int *__restrict__ out, size_t ld_out,
                                                            int metric, int max_dist, int upper, uvaia_gpu_pair *__restrict__ list, unsigned long long list_cap,
                                                            unsigned long long *__restrict__ n_list, int min_compared, uint32_t *parent, unsigned long long *best)
{
  constexpr int RT = PAIRS_CNT_RT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rt = blockIdx.x % n_rtiles, ct = (blockIdx.x / n_rtiles) * 4 + wave;
  if (ct >= n_ctiles) return;
  PairsNear<RT> near;
  if (MODE == PAIRS_NEAR) {
    near.col = (ctile0 + ct) * 64 + lane; near.col_ok = near.col >= col0 && near.col - col0 < n_cols;
    near.row_first = row0 + (long long)rt * RT; near.rows_here = n_rows - rt * RT; near.lane = lane;
    if (near.same(parent, n_list)) return;
  }
  int acc[RT][5];
#pragma unroll
  for (int r = 0; r < RT; r++) { acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = acc[r][4] = 0; }
  const uint4 *t = db + (size_t)(ctile0 + ct) * W4 * 4 * 64 + lane;
  const size_t rstride = (size_t)W4 * PAIRS_CNT_DW;
  const uint32_t *rb = rec + (size_t)rt * RT * rstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    const uint32_t rA[4] = {pA.x, pA.y, pA.z, pA.w}, rC[4] = {pC.x, pC.y, pC.z, pC.w}, rG[4] = {pG.x, pG.y, pG.z, pG.w}, rT[4] = {pT.x, pT.y, pT.z, pT.w};
    uint32_t rv[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rv[j] = rA[j] | rC[j] | rG[j] | rT[j];
      const uint32_t par = rA[j] ^ rC[j] ^ rG[j] ^ rT[j], three = (rA[j] & rC[j] & (rG[j] | rT[j])) | (rG[j] & rT[j] & (rA[j] | rC[j]));
      rs[j] = par & ~three;
    }
    const uint32_t *s0 = rb + (size_t)w4 * PAIRS_CNT_DW;
    QWords<PAIRS_CNT_DW> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int r = 0; r < RT; r++) {
      if (r + 1 < RT) load_qwords(nxt, s0 + (size_t)(r + 1) * rstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t qA = cur.v[j * 6 + 0], qC = cur.v[j * 6 + 1], qG = cur.v[j * 6 + 2], qT_ = cur.v[j * 6 + 3], qv = cur.v[j * 6 + 4], qs = cur.v[j * 6 + 5];
        uint32_t d = rA[j] ^ qA;
        d = B3(rC[j], qC, d, (TT_A ^ TT_B) | TT_C);
        d = B3(rG[j], qG, d, (TT_A ^ TT_B) | TT_C);
        const uint32_t nd = B3(rT[j], qT_, d, ~((TT_A ^ TT_B) | TT_C));   // all four planes equal
        uint32_t x = rA[j] & qA;
        x = B3(rC[j], qC, x, (TT_A & TT_B) | TT_C);
        x = B3(rG[j], qG, x, (TT_A & TT_B) | TT_C);
        x = B3(rT[j], qT_, x, (TT_A & TT_B) | TT_C);                       // sets intersect (implies both valid)
        acc[r][0] = bcnt_acc(nd & qs, acc[r][0]);
        acc[r][1] = bcnt_acc(nd & rv[j], acc[r][1]);
        acc[r][2] = bcnt_acc(x, acc[r][2]);
        acc[r][3] = bcnt_acc(rv[j] & qv, acc[r][3]);
        acc[r][4] = bcnt_acc(rs[j] & qs, acc[r][4]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (r + 1 < RT) cur = nxt;
    }
  }
  const long long col = (ctile0 + ct) * 64 + lane, j = col - col0;
  const bool col_ok = j >= 0 && j < n_cols;
  if (MODE == PAIRS_DENSE) {
    if (!col_ok) return;
#pragma unroll
    for (int r = 0; r < RT; r++) {
      const int i = rt * RT + r;
      if (i < n_rows) {
        int *o = out + ((size_t)i * ld_out + (size_t)j) * UVAIA_GPU_PAIR_NCOUNT;
#pragma unroll
        for (int k = 0; k < UVAIA_GPU_PAIR_NCOUNT; k++) o[k] = acc[r][k];
      }
    }
  } else if (MODE == PAIRS_LINK) {
    uint32_t hits = 0;                                 // bit r: this lane's column is linked to row r of the tile
    unsigned total = 0;                                // wave-uniform: ballots
#pragma unroll
    for (int r = 0; r < RT; r++) {
      const int i = rt * RT + r;
      const bool snp = metric == UVAIA_GPU_DIST_SNP;
      const int c0 = acc[r][0], c2 = acc[r][2], c3 = acc[r][3], c4 = acc[r][4];      // (read first: a choice between two elements would index the accumulators at run time)
      const int dist = snp ? c4 - c0 : c3 - c2, compared = snp ? c4 : c3;
      const bool h = col_ok && i < n_rows && row0 + i < col && dist <= max_dist && compared >= min_compared;
      total += (unsigned)__popcll(__ballot(h));
      hits |= (uint32_t)h << r;
    }
    pairs_link_hits(parent, n_list, (uint32_t)(row0 + rt * RT), (uint32_t)col, hits, total, lane);
  } else if (MODE == PAIRS_NEAR) {
#pragma unroll
    for (int r = 0; r < RT; r++) {
      const bool snp = metric == UVAIA_GPU_DIST_SNP;
      const int c0 = acc[r][0], c2 = acc[r][2], c3 = acc[r][3], c4 = acc[r][4];      // (read first, as the link mode does)
      near.row(r, snp ? c4 - c0 : c3 - c2, (snp ? c4 : c3) >= min_compared);
    }
    near.flush(best);
  } else {
    auto hit = [&](int r) {
      const int i = rt * RT + r;
      const int dist = metric == UVAIA_GPU_DIST_SNP ? acc[r][4] - acc[r][0] : acc[r][3] - acc[r][2];
      return col_ok && i < n_rows && dist <= max_dist && (!upper || row0 + i < col);
    };
    unsigned total = 0;                                // wave-uniform: ballots
#pragma unroll
    for (int r = 0; r < RT; r++) total += (unsigned)__popcll(__ballot(hit(r)));
    if (total == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(n_list, (unsigned long long)total);
    base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RT; r++) {
      const bool h = hit(r);
      const unsigned long long b = __ballot(h);
      const unsigned long long pos = base + (unsigned long long)__popcll(b & below);
      if (h && pos < list_cap) {
        uvaia_gpu_pair p;
        p.row = (uint32_t)(row0 + rt * RT + r); p.col = (uint32_t)col;
#pragma unroll
        for (int k = 0; k < UVAIA_GPU_PAIR_NCOUNT; k++) p.count[k] = acc[r][k];
        list[pos] = p;
      }
      base += (unsigned long long)__popcll(b);
    }
  }
}
