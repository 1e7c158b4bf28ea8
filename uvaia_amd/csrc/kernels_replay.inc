// kernels_replay.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): score assembly, the ordered gate / heap replay.

// ------------------------------------------------------------------------------------------------------------
// device: score assembly and the ordered gate / heap replay
// ------------------------------------------------------------------------------------------------------------
// probes of a -DREPLAY_TIMING build (replay2_kernel, replay3_kernel): wall-clock ticks of a stretch of code added to an accumulator
#ifdef REPLAY_TIMING
#define TT_START(x) const unsigned long long x = wall_clock64()
#define TT_ADD(acc, x) acc += wall_clock64() - x
#else
#define TT_START(x)
#define TT_ADD(acc, x)
#endif
// Assembles score[6] exactly as src/nearest.c:499-501 (default) or :464-469 (--acgt) from
//   cnt = pair counters over all compared columns, rt = untruncated consensus counters over idx_c,
//   rc  = the consensus counters the reference would hold in cq->res (possibly truncated), nn = cq->non_n.
// Pair counters over idx_m + idx are cnt - rt because every query equals the consensus on idx_c.
template <bool ACGT>
static __device__ __forceinline__ void assemble_scores(const int4 cnt, const int4 rt, const int4 rc, int nn, int S[6], int &mism)
{
  if (ACGT) {
    const int pmm = cnt.x - rt.x, pba = cnt.y - rt.y;   // mismatches / comparable sites outside idx_c
    S[0] = (pba + rc.y) - (pmm + rc.x);
    S[1] = pba + rc.y;
    S[2] = S[0] - (rc.y - rc.x);
    S[3] = nn;
    S[4] = rc.x + (pmm - cnt.z);
    S[5] = cnt.z;
    mism = S[1] - S[0];
  } else {
    const int p0 = cnt.x - rt.x;
    S[0] = p0 + rc.x;
    S[1] = cnt.y - rt.y + rc.y;
    S[2] = cnt.z - rt.z + rc.z;
    S[3] = cnt.w - rt.w + rc.w;
    S[4] = p0;
    S[5] = nn;
    mism = S[3] - S[0];
  }
}

static __device__ __forceinline__ bool lex_better(const int a[6], const int b[6])
{ // compare_q_item_score(a,b) < 0 (src/min_heap.c:41-47): a ranks strictly ahead of b
#pragma unroll
  for (int i = 0; i < 6; i++) { if (a[i] != b[i]) return a[i] > b[i]; }
  return false;
}

static __device__ void heap_sift_down(int *h, int n, int p)
{ // heap_bubble_down, src/min_heap.c:119-133: root = worst; swap towards the worse child while p is better than it
  for (;;) {
    int c = 2 * p, pick = p;
    for (int i = 0; i < 2; i++) if (c + i <= n && lex_better(h + pick * HEAP_ENTRY, h + (c + i) * HEAP_ENTRY)) pick = c + i;
    if (pick == p) return;
    for (int i = 0; i < HEAP_ENTRY; i++) { int tmp = h[p * HEAP_ENTRY + i]; h[p * HEAP_ENTRY + i] = h[pick * HEAP_ENTRY + i]; h[pick * HEAP_ENTRY + i] = tmp; }
    p = pick;
  }
}

static __device__ void heap_sift_up(int *h, int i)
{ // heap_bubble_up, src/min_heap.c:135-147
  while (i > 1) {
    const int parent = i / 2;
    if (!lex_better(h + parent * HEAP_ENTRY, h + i * HEAP_ENTRY)) return;
    for (int k = 0; k < HEAP_ENTRY; k++) { int tmp = h[parent * HEAP_ENTRY + k]; h[parent * HEAP_ENTRY + k] = h[i * HEAP_ENTRY + k]; h[i * HEAP_ENTRY + k] = tmp; }
    i = parent;
  }
}

template <bool ACGT> static __device__ __forceinline__ int entry_mismatches(const int *e)
{ return ACGT ? (e[1] - e[0]) : (e[3] - e[0]); }   // src/nearest.c:475 / :508

static __device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// One wave per query.  The wave reads 64 consecutive pair counters of its query at a time, filters them with
// bounds that can only tighten (T_ub = max mismatches held + 1, W = worst kept key: see DESIGN.md "gate"), and
// serialises the survivors in reference order through the exact test of src/nearest.c:488-508.
template <bool ACGT>
__global__ __launch_bounds__(64) void replay_kernel(const int4 *__restrict__ cnt, int ppad, const int4 *__restrict__ rt, const int4 *__restrict__ tr,
                                                     const int *__restrict__ nonn, int r_begin, int r_end, long long ord_base,
                                                     int *__restrict__ heap_g, int *__restrict__ n_g, int *__restrict__ T_g,
                                                     const int *__restrict__ snap_ptr, uint8_t *__restrict__ entered, int k)
{
  extern __shared__ int h[];                 // (k+1) entries of HEAP_ENTRY ints, slot 0 unused
  const int q = blockIdx.x, lane = threadIdx.x;
  int *hg = heap_g + (size_t)q * (k + 1) * HEAP_ENTRY;
  int n = n_g[q], T = T_g[q];
  const int snap = *snap_ptr;
  for (int i = lane; i < (n + 1) * HEAP_ENTRY; i += 64) h[i] = hg[i];
  __syncthreads();
  bool full = (n == k);
  int W[6] = {0, 0, 0, 0, 0, 0};
  int Tub = T;
  if (full) {
    int mx = 0;
    for (int s = 1 + lane; s <= n; s += 64) mx = max(mx, entry_mismatches<ACGT>(h + s * HEAP_ENTRY));
    Tub = wave_max(mx) + 1;
#pragma unroll
    for (int i = 0; i < 6; i++) W[i] = h[HEAP_ENTRY + i];
  }
  const int4 *crow = cnt + (size_t)q * ppad;
  bool dirty = false;
  for (int base = r_begin; base < r_end; base += 64) {
    const int r = base + lane;
    const bool valid = r < r_end;
    int S[6] = {0, 0, 0, 0, 0, 0}, m = 0x7fffffff;
    if (valid) {
      const int4 c = crow[r], a = rt[r];
      const int mc_true = ACGT ? a.x : (a.w - a.x);
      const int4 rc = (mc_true >= snap) ? tr[r] : a;     // what cq->res holds after src/nearest.c:431-432
      assemble_scores<ACGT>(c, a, rc, nonn[r], S, m);
    }
    bool cand = valid && m < Tub && (!full || lex_better(S, W));
    unsigned long long mask = __ballot(cand);
    while (mask) {
      const int i = __ffsll((long long)mask) - 1;
      int Si[6];
#pragma unroll
      for (int s = 0; s < 6; s++) Si[s] = __shfl(S[s], i);
      const int mi = __shfl(m, i);
      const bool accept = (mi < T) && (!full || lex_better(Si, W));   // src/nearest.c:488-496 + heap_insert :93-117
      if (!accept) { mask &= mask - 1; continue; }
      if (lane == 0) {
        const long long ord = ord_base + (base + i - r_begin);
        const int slot = full ? 1 : n + 1;
        int *e = h + slot * HEAP_ENTRY;
#pragma unroll
        for (int s = 0; s < 6; s++) e[s] = Si[s];
        e[6] = (int)(unsigned)(ord & 0xffffffffll); e[7] = (int)(ord >> 32);
        if (full) heap_sift_down(h, n, 1); else heap_sift_up(h, n + 1);
        entered[base + i] = 1;
      }
      if (!full) n++;
      dirty = true;
      __syncthreads();
      const bool was_full = full;
      full = (n == k);
      if (full) {
#pragma unroll
        for (int s = 0; s < 6; s++) W[s] = h[HEAP_ENTRY + s];
        T = entry_mismatches<ACGT>(W) + 1;               // src/nearest.c:506-508 / :474-475
        if (!was_full) {
          int mx = 0;
          for (int s = 1 + lane; s <= n; s += 64) mx = max(mx, entry_mismatches<ACGT>(h + s * HEAP_ENTRY));
          Tub = wave_max(mx) + 1;
        }
      }
      cand = valid && lane > i && m < Tub && (!full || lex_better(S, W));
      mask = __ballot(cand);
    }
  }
  if (dirty) {
    __syncthreads();
    for (int i = lane; i < (n + 1) * HEAP_ENTRY; i += 64) hg[i] = h[i];
    if (lane == 0) { n_g[q] = n; T_g[q] = T; }
  }
}

// ---- wave-cooperative heap operations (same comparisons and swaps as heap_sift_down/up above, hence the same layout):
// lanes 0..7 each hold one of the 8 ints of an entry, the lexicographic compare is a ballot + first-set-bit, a swap is one
// parallel read and write.  Every lane of the wave must call these (uniform control flow); h lives in LDS.
static __device__ __forceinline__ bool wave_entry_better(const int *h, int a, int b, int lane)
{ // entry a ranks strictly ahead of entry b
  const int i = lane & 7;
  const int va = h[a * HEAP_ENTRY + i], vb = h[b * HEAP_ENTRY + i];
  const unsigned long long m = __ballot((i < 6) && (va != vb)) & 0xFFull;
  if (!m) return false;
  const int first = __ffsll((long long)m) - 1;
  return __builtin_amdgcn_readlane(va, first) > __builtin_amdgcn_readlane(vb, first);
}

static __device__ __forceinline__ void wave_entry_swap(int *h, int a, int b, int lane)
{
  if (lane < HEAP_ENTRY) {
    const int va = h[a * HEAP_ENTRY + lane], vb = h[b * HEAP_ENTRY + lane];
    h[a * HEAP_ENTRY + lane] = vb; h[b * HEAP_ENTRY + lane] = va;
  }
  __syncthreads();     // one wave per block: an LDS fence + wave barrier
}

static __device__ void wave_sift_down(int *h, int n, int p, int lane)
{ // src/min_heap.c:119-133
  for (;;) {
    const int c = 2 * p;
    int pick = p;
    if (c <= n && wave_entry_better(h, pick, c, lane)) pick = c;
    if (c + 1 <= n && wave_entry_better(h, pick, c + 1, lane)) pick = c + 1;
    if (pick == p) return;
    wave_entry_swap(h, p, pick, lane);
    p = pick;
  }
}

// Root replacement for a full heap: the same comparisons and the same final layout as "overwrite slot 1, sift down"
// (src/min_heap.c:93-133), but the incoming entry stays in registers (`ment`: lanes l and l+8 hold its int l, l < 8) while
// the children on its way move up: per level one 64-byte LDS read (both children side by side in lanes 0-15), two
// lexicographic compares done with ballots and a DPP row shift, one 32-byte write.  No barrier inside: one wave, LDS
// operations of a wave complete in order.
static __device__ void wave_replace_root(int *h, int n, int ment, int lane)
{
  int p = 1;
  for (;;) {
    const int c = 2 * p;
    if (c > n) break;
    int v = 0;
    if (lane < 16 && c + (lane >> 3) <= n) v = h[c * HEAP_ENTRY + lane];               // lanes 0-7: child c, lanes 8-15: child c + 1
    const unsigned long long ne1 = __ballot(lane < 6 && ment != v), gt1 = __ballot(lane < 6 && ment > v);
    const bool b1 = ne1 && ((gt1 >> (__ffsll((long long)ne1) - 1)) & 1ull);             // the entry ranks strictly ahead of child c
    const int c1up = __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);         // row_shr:8 -> lanes 8-15 see child c
    const int pk = b1 ? c1up : ment;                                                    // lanes 8-13: keys of the pick so far
    const unsigned long long ne2 = __ballot(lane >= 8 && lane < 14 && pk != v), gt2 = __ballot(lane >= 8 && lane < 14 && pk > v);
    const bool b2 = (c + 1 <= n) && ne2 && ((gt2 >> (__ffsll((long long)ne2) - 1)) & 1ull);   // ... strictly ahead of child c + 1
    if (!b1 && !b2) break;
    const int c2dn = __builtin_amdgcn_update_dpp(0, v, 0x108, 0xF, 0xF, false);         // row_shl:8 -> lanes 0-7 see child c + 1
    if (lane < HEAP_ENTRY) h[p * HEAP_ENTRY + lane] = b2 ? c2dn : v;
    p = b2 ? c + 1 : c;
  }
  if (lane < HEAP_ENTRY) h[p * HEAP_ENTRY + lane] = ment;
  __builtin_amdgcn_wave_barrier();
}

// ---- root replacement without the level-by-level chain (heaps of at most 127 entries: every inner node has a lane).
// heap_bubble_down (src/min_heap.c:119-133) moves the new entry x down from the root, at every node towards the WORSE child (ties: the
// left one), for as long as x ranks strictly ahead of that child.  Which child is the worse one does not depend on x: the path from
// the root is known beforehand.  `mc` keeps, in lane p, the worse child of inner node p (0 for leaves and lane 0).  An update is then:
// the path by v_readlane, ONE LDS read of the path's entries (eight lanes each), x against all of them at once (two ballots), the
// entries above x's resting place move up one level in one LDS write, and the min-child lanes of the nodes whose child changed are
// refreshed from one more read.  Same comparisons' outcomes, same final layout as wave_replace_root; W receives the new root's keys.
static __device__ __forceinline__ int wave_minchild_init(const int *h, int n, int lane)
{
  int mcv = 0;
  const int c = 2 * lane;
  if (lane >= 1 && c <= n) {
    mcv = c;
    if (c + 1 <= n) {
      bool decided = false, better = false;
#pragma unroll
      for (int i = 0; i < 6; i++) { const int a = h[c * HEAP_ENTRY + i], b = h[(c + 1) * HEAP_ENTRY + i]; if (!decided && a != b) { decided = true; better = a > b; } }
      if (better) mcv = c + 1;
    }
  }
  return mcv;
}

static __device__ __forceinline__ void wave_replace_root_mc(int *h, int n, int ment /* every lane: int (lane & 7) of the new entry */, int &mc, int lane, int (&W)[6], const int (&Si)[6])
{
  int path[6];                                                     // node at depth d + 1 on the worse-child path, 0 past its end
  {
    int cur = 1;
#pragma unroll
    for (int d = 0; d < 6; d++) { cur = __builtin_amdgcn_readlane(mc, cur); path[d] = cur; }      // (lane 0 and leaves hold 0)
  }
  const int g = lane >> 3, i = lane & 7;
  int pv = 0;
#pragma unroll
  for (int d = 0; d < 6; d++) if (g == d) pv = path[d];
  int v = 0;
  if (pv) v = h[pv * HEAP_ENTRY + i];
  const unsigned long long ne = __ballot(i < 6 && pv != 0 && ment != v), gt = __ballot(i < 6 && pv != 0 && ment > v);
  int D = 0;                                                       // levels the new entry moves down
#pragma unroll
  for (int d = 0; d < 6; d++) {
    const unsigned nb = (unsigned)(ne >> (8 * d)) & 0x3Fu;
    const bool ahead = path[d] != 0 && nb != 0u && ((gt >> (8 * d + (__ffs((int)nb) - 1))) & 1ull);
    if (D == d && ahead) D = d + 1;
  }
  if (g < D) h[(pv >> 1) * HEAP_ENTRY + i] = v;                    // the entries on the way move up to their parents
  const int place = D ? path[D - 1 < 0 ? 0 : D - 1] : 1;
  if (g == 7) h[place * HEAP_ENTRY + i] = ment;
#pragma unroll
  for (int s_ = 0; s_ < 6; s_++) W[s_] = D ? __builtin_amdgcn_readlane(v, s_) : Si[s_];      // the new root: what sat at path[0], or the new entry itself
  // worse child of the nodes whose child on the path changed: the parents of path[0 .. D - 1]
  if (D) {
    const int node = pv >> 1, c = 2 * node;
    int a = 0, b = 0;
    const bool two = g < D && c + 1 <= n;
    if (g < D) { a = h[c * HEAP_ENTRY + i]; b = two ? h[(c + 1) * HEAP_ENTRY + i] : a; }
    const unsigned long long ne2 = __ballot(g < D && i < 6 && a != b), gt2 = __ballot(g < D && i < 6 && a > b);
#pragma unroll
    for (int d = 0; d < 6; d++) {
      if (d < D) {
        const int nd = d ? path[d - 1] : 1, cc = 2 * nd;
        const unsigned nb = (unsigned)(ne2 >> (8 * d)) & 0x3Fu;
        const bool left_ahead = nb != 0u && ((gt2 >> (8 * d + (__ffs((int)nb) - 1))) & 1ull);
        if (lane == nd) mc = left_ahead ? cc + 1 : cc;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// sum over the wave by DPP (row shifts, then row broadcasts): six VALU steps instead of six LDS-crossbar shuffles
static __device__ __forceinline__ int wave_sum_dpp(int v)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);    // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);    // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);    // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);    // row_shr:8  -> lane 15 of every row holds the row's sum
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);    // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);    // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

static __device__ void wave_sift_up(int *h, int i, int lane)
{ // src/min_heap.c:135-147
  while (i > 1) {
    const int parent = i / 2;
    if (!wave_entry_better(h, parent, i, lane)) return;
    wave_entry_swap(h, parent, i, lane);
    i = parent;
  }
}

// ---- on-demand counters for the pairs that reach the heap -------------------------------------------------------
static __device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// contribution of one alignment word to  d1 = #(equal & valid & not ACGT)  and  d2 = #(sets intersect & not equal)
static __device__ __forceinline__ void iupac_word_extra(const uint32_t *__restrict__ dbw, size_t tile_abs, int lane_r, int W4, const uint32_t *__restrict__ qrow6,
                                                        int w, int &d1, int &d2)
{
  const size_t base = (((size_t)tile_abs * W4 + (w >> 2)) * 4) * 256 + (size_t)lane_r * 4 + (w & 3);   // u32 index of plane 0
  const uint32_t rA = dbw[base], rC = dbw[base + 256], rG = dbw[base + 512], rT = dbw[base + 768];
  const uint32_t *s = qrow6 + (size_t)w * 6;
  const uint32_t qA = s[0], qC = s[1], qG = s[2], qT_ = s[3], qa = s[5];
  const uint32_t rv = rA | rC | rG | rT;
  const uint32_t nd = ~((rA ^ qA) | (rC ^ qC) | (rG ^ qG) | (rT ^ qT_));
  const uint32_t e = nd & rv, a0 = nd & qa, x = (rA & qA) | (rC & qC) | (rG & qG) | (rT & qT_);
  d1 += __popc(e & ~a0);
  d2 += __popc(x & ~e);
}

// Default mode: text_matches - ACGT_matches and partial_matches - text_matches of one pair.  Both differences live on
// sites where the query or the reference carries a partially ambiguous code, so only the alignment words listed for
// either sequence are visited (all words if a list overflowed).  Whole wave cooperates; result in every lane.
// (one word's contribution given both sets of four planes: iupac_planes_extra, kernels_scan2.inc)

// Single round trip: the reference's side row (count, listed words and their planes) is one coalesced 256-B load, the
// reference planes at the query's listed words are requested at the same time (they do not depend on the row), and the
// query's planes come from `qw` (LDS copy of its row when it fits, else global memory).  The request is split from its use
// so that the replay can have the rows of the next candidates in flight while it works on the heap.
// Roles by lane: lanes 0..nq-1 take the query's listed words (reference planes gathered from the database tile), lanes
// nq..nq+AMB_CAP-1 the reference's listed words (index and planes straight from its side row), every lane the row's count.
struct ExtraReq { int row /* --acgt: dist_unique; default: the reference's count */; int w; uint32_t rA, rC, rG, rT; int nn; };

static __device__ __forceinline__ ExtraReq wave_iupac_request(const uint4 *__restrict__ db, size_t tile_abs, int lane_r, int W4, const int *__restrict__ ref_row,
                                                              int nq, int wq, int lane)
{
  const uint32_t *dbw = reinterpret_cast<const uint32_t *>(db);
  ExtraReq e;
  e.row = ref_row[0];
  e.w = -1; e.rA = e.rC = e.rG = e.rT = 0u; e.nn = 0;
  if (nq <= AMB_CAP) {
    if (lane < nq) {
      const size_t base = (((size_t)tile_abs * W4 + (wq >> 2)) * 4) * 256 + (size_t)lane_r * 4 + (wq & 3);
      e.w = wq; e.rA = dbw[base]; e.rC = dbw[base + 256]; e.rG = dbw[base + 512]; e.rT = dbw[base + 768];
    } else if (lane < nq + AMB_CAP) {
      const int kr = lane - nq;
      const int4 pl = *reinterpret_cast<const int4 *>(ref_row + 12 + 4 * kr);
      e.w = ref_row[1 + kr]; e.rA = (uint32_t)pl.x; e.rC = (uint32_t)pl.y; e.rG = (uint32_t)pl.z; e.rT = (uint32_t)pl.w;
    }
  }
  return e;
}

static __device__ int2 wave_iupac_finish(const ExtraReq &e, const uint4 *__restrict__ db, size_t tile_abs, int lane_r, int W4, const uint32_t *qw,
                                         const uint32_t *qlisted /*LDS bitmap of the words the query lists*/, int nq, int lane, bool &dense)
{
  const uint32_t *dbw = reinterpret_cast<const uint32_t *>(db);
  const int nr = e.row;
  dense = (nr > AMB_CAP || nq > AMB_CAP);
  if (!dense) {
    int pk = 0;
    // the reference's words the query lists itself are already covered by the query's lanes
    const bool mine = lane < nq || (lane < nq + nr && !((qlisted[e.w >> 5] >> (e.w & 31)) & 1u));
    if (mine) {
      const uint32_t *sq = qw + (size_t)e.w * 6;
      int d1 = 0, d2 = 0;
      iupac_planes_extra(e.rA, e.rC, e.rG, e.rT, sq[0], sq[1], sq[2], sq[3], sq[5], d1, d2);
      pk = d1 | (d2 << 16);                                   // at most 64 x 32 per half
    }
    const int tot = wave_sum_dpp(pk);
    return make_int2(tot & 0xFFFF, (int)((unsigned)tot >> 16));
  }
  int d1 = 0, d2 = 0;
  for (int w = lane; w < W4 * 4; w += 64) {
    const size_t base = (((size_t)tile_abs * W4 + (w >> 2)) * 4) * 256 + (size_t)lane_r * 4 + (w & 3);
    const uint32_t *sq = qw + (size_t)w * 6;
    iupac_planes_extra(dbw[base], dbw[base + 256], dbw[base + 512], dbw[base + 768], sq[0], sq[1], sq[2], sq[3], sq[5], d1, d2);
  }
  return make_int2(wave_sum(d1), wave_sum(d2));
}

// --acgt mode: mismatches on the polymorphic query columns (score[5], src/nearest.c:469) of one pair, dense.
static __device__ int wave_acgt_poly_mismatches(const uint4 *__restrict__ db, size_t tile_abs, int lane_r, int W4, const uint32_t *__restrict__ qrow4, int lane)
{
  int mp = 0;
  for (int w4 = lane; w4 < W4; w4 += 64) {
    const uint4 *t = db + ((size_t)tile_abs * W4 + w4) * 3 * 64 + lane_r;
    const uint4 pL = t[0], pH = t[64], pI = t[128];
    const uint32_t *s = qrow4 + (size_t)w4 * 16;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t y = ((&pL.x)[j] ^ s[j * 4 + 0]) | ((&pH.x)[j] ^ s[j * 4 + 1]);
      mp += __popc(y & (&pI.x)[j] & s[j * 4 + 3]);
    }
  }
  return wave_sum(mp);
}

// --acgt with rare columns: the scan's dense count covers the truly polymorphic columns only; the mismatches of one pair on the
// rare columns (which belong to dist_unique as well) are counted here on the gathered planes: NR4 * 4 words, one per lane.
static __device__ int wave_rare_mismatches(const uint4 *__restrict__ polyp, size_t tile_abs, int lane_r, int NPT, int NP4, int NR4,
                                           const uint32_t *__restrict__ qr /* [NR4 * 4][lo, hi, isACGT] */, int lane)
{
  const uint32_t *pw = reinterpret_cast<const uint32_t *>(polyp);
  int mp = 0;
  for (int w = lane; w < NR4 * 4; w += 64) {
    const size_t base = (((size_t)tile_abs * NPT + NP4 + (w >> 2)) * 3) * 256 + (size_t)lane_r * 4 + (w & 3);
    const uint32_t rL = pw[base], rH = pw[base + 256], rI = pw[base + 512];
    const uint32_t *s_ = qr + (size_t)w * 3;
    mp += __popc(((rL ^ s_[0]) | (rH ^ s_[1])) & rI & s_[2]);
  }
  return wave_sum_dpp(mp);
}

// --acgt, column-compressed scan: the pair's mismatches on the densely counted polymorphic columns (the other part of dist_unique),
// on the gathered planes: NP4 * 4 words, one per lane, against the query's compressed planes qpl[p4][lo, hi, isACGT, -][4].
static __device__ int wave_dense_poly_mismatches(const uint4 *__restrict__ polyp, size_t tile_abs, int lane_r, int NPT, int NP4, const uint32_t *__restrict__ qpl_row, int lane)
{
  const uint32_t *pw = reinterpret_cast<const uint32_t *>(polyp);
  int mp = 0;
  for (int w = lane; w < NP4 * 4; w += 64) {
    const size_t base = (((size_t)tile_abs * NPT + (w >> 2)) * 3) * 256 + (size_t)lane_r * 4 + (w & 3);
    const uint32_t rL = pw[base], rH = pw[base + 256], rI = pw[base + 512];
    const uint32_t *s_ = qpl_row + (size_t)(w >> 2) * 16 + (w & 3);
    mp += __popc(((rL ^ s_[0]) | (rH ^ s_[4])) & rI & s_[8]);
  }
  return wave_sum_dpp(mp);
}

// ---- what replay2_kernel, replay2_lean_kernel and replay3_kernel share: the state of a query's heap around the walk, the exact
// evaluation of a default-mode candidate and the admission.  One wave per block, uniform control flow; the barriers are counted in
// the comments because each kernel keeps the ones it had.  LEAN (replay2_lean_kernel): what is uniform over the wave is forced into
// scalars (v_readfirstlane), and the heap has at most 127 entries.
template <bool LEAN> static __device__ __forceinline__ void replay_worst_keys(const int *h, int (&W)[6])
{ // the keys of the root (the worst kept entry)
#pragma unroll
  for (int i = 0; i < 6; i++) W[i] = LEAN ? __builtin_amdgcn_readfirstlane(h[HEAP_ENTRY + i]) : h[HEAP_ENTRY + i];
}

// the heap of a query from memory into LDS, no barrier: the caller's next one publishes it.  Returns the clamped entry count.
static __device__ __forceinline__ int replay_load_heap(int *h, const int *__restrict__ hg, int n_stored, int k, int lane)
{
  const int n = min(max(n_stored, 0), k);           // clamp: an imported state blob is external input
  for (int i = lane; i < (n + 1) * HEAP_ENTRY; i += 64) h[i] = hg[i];
  return n;
}

// full, W and mc of the heap in LDS (behind a barrier after replay_load_heap); returns use_mc
template <bool LEAN> static __device__ __forceinline__ bool replay_heap_state(const int *h, int n, int k, int lane, bool &full, int (&W)[6], int &mc)
{
  const bool use_mc = k <= 127;                     // every inner node of the heap has a lane: root replacement along the worse-child path (wave_replace_root_mc)
  full = (n == k);
#pragma unroll
  for (int i = 0; i < 6; i++) W[i] = 0;
  mc = 0;
  if (full) {
    replay_worst_keys<LEAN>(h, W);
    if (LEAN || use_mc) mc = wave_minchild_init(h, n, lane);
  }
  return LEAN || use_mc;
}

// The query's ambiguity-word list, one int per lane: how many words it lists (aq_n), lane l's listed word (aq_w), and the 32-word LDS
// bitmap of the listed words.  Two barriers: the first one also publishes what the caller wrote to LDS before the call.
template <bool LEAN> static __device__ __forceinline__ void replay_query_listed(const int *__restrict__ amb_q, int q, int lane, uint32_t *qlisted, int &aq_n, int &aq_w)
{
  const int aqv = (lane < AMB_STRIDE) ? amb_q[(size_t)q * AMB_STRIDE + lane] : 0;
  aq_n = LEAN ? __builtin_amdgcn_readlane(aqv, 0) : __shfl(aqv, 0);
  aq_w = __shfl(aqv, 1 + ((lane < aq_n && lane < AMB_CAP) ? lane : 0));
  if (lane < 32) qlisted[lane] = 0u;
  __syncthreads();
  if (lane < aq_n && aq_n <= AMB_CAP) atomicOr(&qlisted[aq_w >> 5], 1u << (aq_w & 31));
  __syncthreads();
}

// the end of a replay: heap, entry count and tolerance back to memory if an admission changed them (one barrier), the counters to `stats`
static __device__ __forceinline__ void replay_store_state(const int *h, int *__restrict__ hg, int *__restrict__ n_g, int *__restrict__ T_g, int q, int n, int T, bool dirty,
                                                          unsigned long long *__restrict__ stats, unsigned n_admit, unsigned n_demand, unsigned n_dense, int lane)
{
  if (dirty) {
    __syncthreads();
    for (int i = lane; i < (n + 1) * HEAP_ENTRY; i += 64) hg[i] = h[i];
    if (lane == 0) { n_g[q] = n; T_g[q] = T; }
  }
  if (stats && lane == 0) { atomicAdd(&stats[0], (unsigned long long)n_admit); atomicAdd(&stats[1], (unsigned long long)n_demand); atomicAdd(&stats[2], (unsigned long long)n_dense); }
}

// Bounds of the next 64-tile rounds, requested PD rounds ahead (replay2_kernel, replay2_lean_kernel): with few queries (a handful of
// waves next to a scan that saturates HBM) the walk over the bounds is a chain of dependent loads, and most rounds need nothing but
// their bounds.  Lane l holds tile l of each round: smallest mismatch count (.x), largest first key (.y).
constexpr int PD = 4;
static __device__ __forceinline__ void replay_bounds_start(int2 (&nbq)[PD], const int2 *__restrict__ tmrow, bool use_tmin, int n_slice_tiles, int lane)
{
#pragma unroll
  for (int i = 0; i < PD; i++) { nbq[i] = make_int2(-1, 0x7fffffff); if (use_tmin && i * 64 + lane < n_slice_tiles) nbq[i] = tmrow[i * 64 + lane]; }
}

// the bounds of round tb / 64 (0x7fffffff twice for a tile past the slice); the queue moves up and round tb / 64 + PD is requested
static __device__ __forceinline__ int2 replay_bounds_next(int2 (&nbq)[PD], const int2 *__restrict__ tmrow, bool use_tmin, int n_slice_tiles, int tb, int lane)
{
  int2 b = make_int2(0x7fffffff, 0x7fffffff);
  if (tb + lane < n_slice_tiles) b = nbq[0];
#pragma unroll
  for (int i = 0; i + 1 < PD; i++) nbq[i] = nbq[i + 1];
  if (use_tmin && tb + PD * 64 + lane < n_slice_tiles) nbq[PD - 1] = tmrow[tb + PD * 64 + lane];
  return b;
}

// Exact evaluation of a default-mode candidate whose on-demand words were requested (`cur`): its other two counters, score[] as
// src/nearest.c:499-501 assembles it, the test of src/nearest.c:488-496 + heap_insert (src/min_heap.c:93-117).  cx, cy: the pair's two scan
// counters; ai, ri: its consensus counters, untruncated and as cq->res holds them; nni: the reference's valid sites.
template <bool LEAN>
static __device__ __forceinline__ bool replay_exact_default(const ExtraReq &cur, const uint4 *__restrict__ db, size_t tile_abs, int lane_r, int W4, const uint32_t *qw, const uint32_t *qlisted,
                                                            int aq_n, int lane, int cx, int cy, const int4 ai, const int4 ri, int nni, int T, bool full, const int (&W)[6],
                                                            int (&Si)[6], unsigned &n_dense)
{
  bool dense;
  int2 d = wave_iupac_finish(cur, db, tile_abs, lane_r, W4, qw, qlisted, aq_n, lane, dense);
  n_dense += dense;
  if (LEAN) d = make_int2(__builtin_amdgcn_readfirstlane(d.x), __builtin_amdgcn_readfirstlane(d.y));
  int mi;
  assemble_scores<false>(make_int4(cx, cx + d.x, cx + d.x + d.y, cy), ai, ri, nni, Si, mi);
  const bool accept = (mi < T) && (!full || lex_better(Si, W));
  return accept;
}

// Admission of the accepted candidate `rl` (index relative to the first tile of the batch) with scores Si: the entry built in lanes 0-7
// and 8-15, its entered flag, the heap update -- root replacement along the worse-child path (use_mc), level by level (larger heaps), or
// append + sift-up while the heap fills: the comparisons and swaps of src/min_heap.c:93-147, hence its layout --, then (behind a barrier)
// full, the worst kept keys W unless wave_replace_root_mc left them, the worse-child lanes on the first fill, and the tolerance.
template <bool ACGT, bool LEAN>
static __device__ __forceinline__ void replay_admit(int *h, int k, int &n, int &T, bool &full, int (&W)[6], int &mc, const bool use_mc, const int (&Si)[6],
                                                    long long ord_base, int r_begin, int rl, uint8_t *__restrict__ entered, int lane)
{
  const long long ord = ord_base + (rl - r_begin);
  int v = (int)(unsigned)(ord & 0xffffffffll);                   // lanes l and l + 8 hold int l of the new entry
  if ((lane & 7) == 7) v = (int)(ord >> 32);
#pragma unroll
  for (int sidx = 0; sidx < 6; sidx++) if ((lane & 7) == sidx) v = Si[sidx];
  if (lane == 0) entered[rl] = 1;
  if (full && use_mc) wave_replace_root_mc(h, n, v, mc, lane, W, Si);      // (leaves the new root's keys in W)
  else if (full) wave_replace_root(h, n, v, lane);
  else {
    if (lane < HEAP_ENTRY) h[(n + 1) * HEAP_ENTRY + lane] = v;
    __syncthreads();
    wave_sift_up(h, n + 1, lane);
  }
  const bool was_full = full;
  if (!full) n++;
  __syncthreads();
  full = (n == k);
  if (full) {
    if (!(was_full && use_mc)) replay_worst_keys<LEAN>(h, W);
    if (!was_full && use_mc) mc = wave_minchild_init(h, n, lane);
    T = entry_mismatches<ACGT>(W) + 1;                             // src/nearest.c:506-508 / :474-475
  }
}

// Replay over the two-counter scan.  One wave per query walks the batch in reference order, 256 references per
// round.  Between two admissions the heap state is constant, so the exact tests of src/nearest.c:488-496 and
// src/min_heap.c:95 are evaluated for 64 references at once (ballot); the first survivor in order gets its missing
// counters on demand, is compared exactly, and if admitted the remaining lanes are re-tested against the new state.
// CONS = false: no column is constant and complete (query->n_idx_c == 0), every consensus counter is zero and is not loaded;
// in default mode valid_ref_sites (key 5) is then fetched only for the pairs that reach the exact compare.
template <bool ACGT, bool CONS, int PFN = 3 /* candidates of a tile whose on-demand data are requested ahead */>
__global__ __launch_bounds__(64) void replay2_kernel(const uint32_t *__restrict__ cnt /* first | second << 16 per pair */, int ppad, const int4 *__restrict__ rt, const uint32_t *__restrict__ cp_cons /* consensus planes on idx_c */,
                                                      const int *__restrict__ nonn, const int *__restrict__ amb, int r_begin, int r_end, long long ord_base,
                                                      int *__restrict__ heap_g, int *__restrict__ n_g, int *__restrict__ T_g,
                                                      const int *__restrict__ snap_ptr, uint8_t *__restrict__ entered, int k,
                                                      const uint4 *__restrict__ db, long long tile_first, int W4,
                                                      const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q,
                                                      unsigned long long *__restrict__ stats, int q_first, const int2 *__restrict__ tmin,
                                                      const uint32_t *__restrict__ qpl /* column-compressed scan: the queries' compressed polymorphic planes; else null */, int lq_words, int prio_,
                                                      const uint4 *__restrict__ polyp, int NPT, int NP4, int NR4, const uint32_t *__restrict__ qrare)
{
  extern __shared__ int h[];
  if (prio_) __builtin_amdgcn_s_setprio(3);     // few latency-bound waves on the critical path: win issue arbitration against co-resident scan waves
  const int q = blockIdx.x + q_first, lane = threadIdx.x;
  int *hg = heap_g + (size_t)q * (k + 1) * HEAP_ENTRY;
  int n = replay_load_heap(h, hg, n_g[q], k, lane), T = T_g[q];
  const int snap = *snap_ptr;
  __syncthreads();
  bool full;
  int W[6], mc;
  const bool use_mc = replay_heap_state<false>(h, n, k, lane, full, W, mc);
  const uint32_t *crow = cnt + (size_t)q * ppad;
  const uint32_t *qrow = qfull + (size_t)q * W4 * 4 * (ACGT ? 4 : 6);
  // default mode: keep the query's full planes in LDS (behind the heap) when they fit; the on-demand counters then need a
  // single global round trip per pair
  const uint32_t *qw = qrow;
  if (!ACGT && lq_words > 0) {
    uint32_t *lq = reinterpret_cast<uint32_t *>(h + (k + 1) * HEAP_ENTRY);
    for (int i = lane; i < lq_words; i += 64) lq[i] = qrow[i];
    qw = lq;
  }
  uint32_t *qlisted = reinterpret_cast<uint32_t *>(h + (k + 1) * HEAP_ENTRY) + lq_words;   // 32-word bitmap of the listed words
  int aq_n, aq_w;
  replay_query_listed<false>(amb_q, q, lane, qlisted, aq_n, aq_w);
  bool dirty = false;
  unsigned n_admit = 0, n_demand = 0, n_dense = 0;
#ifdef REPLAY_TIMING
  unsigned long long t2_fetch = 0, t2_finish = 0, t2_heap = 0, t2_group = 0, n_trise = 0, n_groups = 0; const unsigned long long t2_begin = wall_clock64();
#endif
  // prefetch: the counters of round i+1 are requested before round i is processed (the kernel is latency bound:
  // one wave per query, a few hundred dependent rounds)
  // Traversal.  Tiles (64 references) whose smallest mismatch count is not below the current tolerance cannot produce an
  // admission, and the tolerance only changes through admissions; so the wave walks the tile minima (64 tiles per load) and
  // fetches pair counters only for tiles that can pass the gate now, four tiles in flight.  After an admission that changed
  // the tolerance the set of needed tiles is derived again (a tile skipped earlier may qualify once the tolerance rises).
  // Exact for any sequence of tolerances.
  const bool use_tmin = tmin != nullptr;
  const int2 *tmrow = use_tmin ? tmin + (size_t)q * (ppad >> 6) : nullptr;
  const int n_slice_tiles = (r_end + 63) >> 6;
  constexpr int D = 8;      // tiles whose counters are in flight (16 and 32 for a handful of queries measured 1.7x and 2x SLOWER in round 3: the bookkeeping of the group, not the latency, bounds the wave)
  int2 nbq[PD];
  replay_bounds_start(nbq, tmrow, use_tmin, n_slice_tiles, lane);
  for (int tb = 0; tb < n_slice_tiles; tb += 64) {
    const int2 tbound = replay_bounds_next(nbq, tmrow, use_tmin, n_slice_tiles, tb, lane);
    const int tm = tbound.x, tk = tbound.y;          // tile bounds: smallest mismatch count, largest first key
    // a tile can admit only if some reference passes the gate and (heap full) some reference's first key reaches the worst kept one
    // With consensus counters (CONS) a pre-score cut short at the snapshot lowers a pair's mismatch count, but never below the
    // snapshot, and never raises its first key: the bounds stay valid with "tm < T" widened to "tm < T or snapshot < T".
    auto needed = [&]() -> unsigned long long { return __ballot((tm < T || (CONS && snap < T)) && (!full || tk >= W[0])); };
    unsigned long long P = needed();
    while (P) {
      int tsel[D]; uint32_t craw[D]; int4 a[D]; int nn[D], m[D], K0[D], K1[D], K2[D], K3[D]; bool valid[D], cut[D];
      {
        unsigned long long rest = P;
#pragma unroll
        for (int i = 0; i < D; i++) { tsel[i] = rest ? (__ffsll((long long)rest) - 1) : -1; rest &= rest - 1; }
      }
#pragma unroll
      for (int i = 0; i < D; i++) {                                    // request the counters of up to D needed tiles
        craw[i] = 0u; a[i] = make_int4(0, 0, 0, 0); nn[i] = 0; valid[i] = false;
        if (tsel[i] >= 0) {
          const int r = (tb + tsel[i]) * 64 + lane;
          valid[i] = (r >= r_begin && r < r_end);
          if (valid[i]) {
            // (unpacked where it is used: nothing here may wait for the load, up to D of them are in flight)
            craw[i] = crow[r];
            if (CONS) a[i] = rt[r];
            if (CONS || ACGT) nn[i] = nonn[r];
          }
        }
      }
      // (Requesting the first candidate of EVERY tile of the group here, all at once -- about half of config[1]'s admissions are a tile's
      // first, each a full round trip in the chain -- was built in round 4 and measured: exact, and the step went from 3.19 to 3.65 ms.  Eight
      // unrolled mask-and-request blocks and 239 registers per wave cost the replay more instructions than the round trips they hide.)
      bool regroup = false;
#ifdef REPLAY_TIMING
      n_groups++;
      { TT_START(tg_); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TT_ADD(t2_group, tg_); }     // what the group's counters cost the chain
#endif
#pragma unroll
      for (int u = 0; u < D; u++) {
        if (tsel[u] < 0 || regroup) continue;
        const int2 cu = make_int2((int)(craw[u] & 0xFFFFu), (int)(craw[u] >> 16));      // first | second << 16
        {
          // A pre-score that reached the snapshot was cut short there (src/nearest.c:431-432): cq->res then holds exactly `snap`
          // mismatches, so the pair's mismatch count is known; its keys are bounded from above by the uncut counters (a cut only
          // takes matches away).  The cut counters themselves are computed for the pairs that reach the exact comparison.
          const int mc_true = ACGT ? a[u].x : (a[u].w - a[u].x);
          cut[u] = CONS && mc_true >= snap;
          if (ACGT) {     // keys 0..3 are known from the two counters: matches, valid, unique matches, valid ref sites
            K1[u] = cu.y;
            K0[u] = K1[u] - cu.x;
            K2[u] = K0[u] - (a[u].y - a[u].x);
            K3[u] = nn[u];
            m[u] = cu.x - (cut[u] ? mc_true - snap : 0);
          } else {        // only key 0 (ACGT matches) and the pair's valid count are known
            K0[u] = cu.x;
            K3[u] = cu.y;
            K1[u] = K2[u] = 0;
            m[u] = K3[u] - K0[u] - (cut[u] ? mc_true - snap : 0);
          }
        }
        const int T_used = T;
        const int base_u = (tb + tsel[u]) * 64;
        auto may_enter = [&]() -> bool {
          if (!valid[u] || m[u] >= T) return false;
          if (!full) return true;
          if (cut[u]) return K0[u] >= W[0];                 // keys of a cut pair: upper bounds until its cut counters are known
          if (ACGT) {
            if (K0[u] != W[0]) return K0[u] > W[0];
            if (K1[u] != W[1]) return K1[u] > W[1];
            if (K2[u] != W[2]) return K2[u] > W[2];
            return K3[u] >= W[3];
          }
          return K0[u] >= W[0];
        };
        unsigned long long mask = __ballot(may_enter());
        // What a candidate needs beyond the two scan counters (side row / dist_unique, valid sites of the reference) is requested
        // for the next PF candidates of the tile while the current one goes through the heap: the requests depend on the
        // reference only, never on the heap state, so a candidate that drops out after an admission merely wastes its request.
        constexpr int PF = PFN;
        int pf_idx[PF]; ExtraReq pf[PF];
#pragma unroll
        for (int s_ = 0; s_ < PF; s_++) pf_idx[s_] = -1;
        auto request = [&](int i_) -> ExtraReq {
          const int rl_ = base_u + i_;
          ExtraReq e;
          if (ACGT) { e.row = 0; e.w = -1; e.rA = e.rC = e.rG = e.rT = 0u; }
          else e = wave_iupac_request(db, (size_t)tile_first + (size_t)(rl_ >> 6), rl_ & 63, W4, amb + (size_t)rl_ * AMB_ROW, aq_n, aq_w, lane);
          e.nn = (CONS || ACGT) ? 0 : nonn[rl_];
          return e;
        };
        while (mask) {
          const int i = __ffsll((long long)mask) - 1;
          {   // keep the first PF candidates of the mask requested
            unsigned long long rest = mask;
#pragma unroll
            for (int d_ = 0; d_ < PF; d_++) {
              if (!rest) break;
              const int ib = __ffsll((long long)rest) - 1; rest &= rest - 1;
              bool have = false;
#pragma unroll
              for (int s_ = 0; s_ < PF; s_++) have |= (pf_idx[s_] == ib);
              if (!have) {
                // free slot: one whose candidate is no longer among the first PF of the mask (or empty)
                // (the tolerance can rise after an admission, so the mask can gain candidates ahead of the ones already requested:
                // with no stale slot, the slot of the farthest candidate is given up)
                int slot = -1, far = 0;
#pragma unroll
                for (int s_ = PF - 1; s_ >= 0; s_--) {
                  if (pf_idx[s_] < 0 || pf_idx[s_] < i || !((mask >> pf_idx[s_]) & 1ull)) slot = s_;
                  if (pf_idx[s_] > pf_idx[far]) far = s_;
                }
                if (slot < 0) slot = far;
                const ExtraReq e = request(ib);
#pragma unroll
                for (int s_ = 0; s_ < PF; s_++) if (s_ == slot) { pf[s_] = e; pf_idx[s_] = ib; }
              }
            }
          }
          ExtraReq cur = pf[0];
#pragma unroll
          for (int s_ = 1; s_ < PF; s_++) if (pf_idx[s_] == i) cur = pf[s_];
#ifdef REPLAY_TIMING
          { TT_START(tf_); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TT_ADD(t2_fetch, tf_); }       // the round trip of this candidate's words
#endif
          TT_START(tfin_);
#pragma unroll
          for (int s_ = 0; s_ < PF; s_++) if (pf_idx[s_] == i) pf_idx[s_] = -1;
          const int rl = base_u + i;                                      // index relative to the first tile of the batch
          // (the candidate's lane is wave-uniform: v_readlane, not a trip through the LDS crossbar per value)
          const int cx = __builtin_amdgcn_readlane(cu.x, i), cy = __builtin_amdgcn_readlane(cu.y, i);
          const int4 ai = CONS ? make_int4(__builtin_amdgcn_readlane(a[u].x, i), __builtin_amdgcn_readlane(a[u].y, i), __builtin_amdgcn_readlane(a[u].z, i), __builtin_amdgcn_readlane(a[u].w, i)) : make_int4(0, 0, 0, 0);
          int4 ri = ai;                                                   // what cq->res holds: the uncut counters, or ...
          const int nni = (CONS || ACGT) ? __builtin_amdgcn_readlane(nn[u], i) : cur.nn;
          const size_t tile_abs = (size_t)tile_first + (size_t)(rl >> 6);
          if (CONS && ((__ballot(cut[u]) >> i) & 1ull)) ri = wave_truncated_consensus<ACGT>(db, tile_abs, rl & 63, W4, cp_cons, snap, lane);   // ... the ones the cut walk returns
          int Si[6];
          bool accept;
          n_demand++;
          if (ACGT) {
            // with the column-compressed scan the dense count on the polymorphic columns IS score[5] (src/nearest.c:469)
            // dist_unique (src/nearest.c:469): with the column-compressed scan from the gathered planes of the polymorphic and the rare columns
            int mp = qpl ? wave_dense_poly_mismatches(polyp, tile_abs, rl & 63, NPT, NP4, qpl + (size_t)q * NP4 * 16, lane) : wave_acgt_poly_mismatches(db, tile_abs, rl & 63, W4, qrow, lane);
            if (qpl && NR4 > 0) mp += wave_rare_mismatches(polyp, tile_abs, rl & 63, NPT, NP4, NR4, qrare + (size_t)q * NR4 * 12, lane);
            int mi;
            assemble_scores<true>(make_int4(cx, cy, mp, 0), ai, ri, nni, Si, mi);
            accept = (mi < T) && (!full || lex_better(Si, W));            // src/nearest.c:488-496 + heap_insert :93-117
          } else accept = replay_exact_default<false>(cur, db, tile_abs, rl & 63, W4, qw, qlisted, aq_n, lane, cx, cy, ai, ri, nni, T, full, W, Si, n_dense);
          TT_ADD(t2_finish, tfin_);
          if (!accept) { mask &= mask - 1; continue; }
          TT_START(th_);
          replay_admit<ACGT, false>(h, k, n, T, full, W, mc, use_mc, Si, ord_base, r_begin, rl, entered, lane);
          dirty = true; n_admit++;
          TT_ADD(t2_heap, th_);
          mask = __ballot(lane > i && may_enter());
        }
#ifdef REPLAY_TIMING
        if (T > T_used) n_trise++;
#endif
        P &= ~(1ull << tsel[u]);                                          // this tile is done
        if (T != T_used) {
          // Needed tiles under the new tolerance, after this one.  A lower tolerance only removes tiles: the ones already in
          // flight are processed anyway (their ballots come out empty).  A higher tolerance can add a tile that lies BEFORE
          // the next tile in flight; only then must the group be formed again to keep the stream order.
          P = needed() & ~((2ull << tsel[u]) - 1ull);
          unsigned long long inflight = 0ull; int last = -1;
#pragma unroll
          for (int v = 0; v < D; v++) if (v > u && tsel[v] >= 0) { inflight |= (1ull << tsel[v]); last = tsel[v]; }
          // a needed tile that is not in flight but precedes the last tile in flight would be visited out of order
          if (T > T_used && last >= 0 && (P & ~inflight & ((1ull << last) - 1ull)) != 0ull) regroup = true;
          else P |= inflight;                                             // keep the tiles in flight in the pending set
        }
      }
    }
  }
  replay_store_state(h, hg, n_g, T_g, q, n, T, dirty, stats, n_admit, n_demand, n_dense, lane);
#ifdef REPLAY_TIMING
  if (stats && lane == 0) { atomicAdd(&stats[4], t2_fetch); atomicAdd(&stats[5], t2_finish); atomicAdd(&stats[6], t2_heap); atomicAdd(&stats[7], t2_group); atomicAdd(&stats[8], n_trise); atomicAdd(&stats[9], n_groups);
                            atomicAdd(&stats[10], wall_clock64() - t2_begin); atomicMax(&stats[11], wall_clock64() - t2_begin); }
#endif
}

// replay2_kernel<false, false, 2> for heaps of at most 127 entries and the query's planes read from memory (no LDS copy): the regime of a
// large query set in default mode without constant-and-complete columns.  The same machine -- the tile bounds select the tiles, D of them in
// flight in stream order, the same ballot, the same exact comparison (wave_iupac_request / wave_iupac_finish, assemble_scores, lex_better),
// the same heap operations --, written so that a wave keeps 128 registers or fewer (DESIGN.md 4.4: one such wave on a SIMD leaves room for
// three blocks of the scan on the compute unit instead of two):
//   * one copy of the per-tile body: the group is a bit mask of the tiles in flight, their counters a queue that moves up by one per tile;
//   * two request slots with fixed roles (`cur`: the candidate at the head of the mask, `nxt`: the one behind it) instead of slots that are
//     searched and matched per candidate;
//   * what is uniform over the wave -- the worst kept keys, the candidate's scores -- is held as scalars;
//   * no argument, array or branch of --acgt, of the consensus pre-score or of the larger heaps.
__global__ __launch_bounds__(64) void replay2_lean_kernel(const uint32_t *__restrict__ cnt /* first | second << 16 per pair */, int ppad, const int *__restrict__ nonn, const int *__restrict__ amb,
                                                           int r_begin, int r_end, long long ord_base, int *__restrict__ heap_g, int *__restrict__ n_g, int *__restrict__ T_g,
                                                           uint8_t *__restrict__ entered, int k /* <= 127 */, const uint4 *__restrict__ db, long long tile_first, int W4,
                                                           const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q, unsigned long long *__restrict__ stats, int q_first,
                                                           const int2 *__restrict__ tmin, int prio_)
{
  extern __shared__ int h[];
  if (prio_) __builtin_amdgcn_s_setprio(3);
  const int q = blockIdx.x + q_first, lane = threadIdx.x;
  int *hg = heap_g + (size_t)q * (k + 1) * HEAP_ENTRY;
  int n = replay_load_heap(h, hg, n_g[q], k, lane), T = T_g[q];
  __syncthreads();
  bool full;
  int W[6], mc;
  replay_heap_state<true>(h, n, k, lane, full, W, mc);
  const uint32_t *crow = cnt + (size_t)q * ppad;
  const uint32_t *qw = qfull + (size_t)q * W4 * 4 * 6;
  uint32_t *qlisted = reinterpret_cast<uint32_t *>(h + (k + 1) * HEAP_ENTRY);           // 32-word bitmap of the listed words
  int aq_n, aq_w;
  replay_query_listed<true>(amb_q, q, lane, qlisted, aq_n, aq_w);
  bool dirty = false;
  unsigned n_admit = 0, n_demand = 0, n_dense = 0;
  const bool use_tmin = tmin != nullptr;
  const int2 *tmrow = use_tmin ? tmin + (size_t)q * (ppad >> 6) : nullptr;
  const int n_slice_tiles = (r_end + 63) >> 6;
  constexpr int D = 8;              // tiles in flight (as replay2_kernel)
  int2 nbq[PD];
  replay_bounds_start(nbq, tmrow, use_tmin, n_slice_tiles, lane);
  for (int tb = 0; tb < n_slice_tiles; tb += 64) {
    const int2 tbound = replay_bounds_next(nbq, tmrow, use_tmin, n_slice_tiles, tb, lane);
    const int tm = tbound.x, tk = tbound.y;          // tile bounds: smallest mismatch count, largest first key
    auto needed = [&]() -> unsigned long long { return __ballot(tm < T && (!full || tk >= W[0])); };
    unsigned long long P = needed();
    while (P) {
      // the group: the first D needed tiles, their counters requested together (unpacked where they are used)
      unsigned long long G;
      uint32_t craw[D];
      {
        unsigned long long rest = P;
#pragma unroll
        for (int i = 0; i < D; i++) {
          craw[i] = 0u;
          if (rest) {
            const int r = (tb + (__ffsll((long long)rest) - 1)) * 64 + lane;
            if (r >= r_begin && r < r_end) craw[i] = crow[r];
            rest &= rest - 1;
          }
        }
        G = P & ~rest;
      }
#pragma unroll 1
      while (G) {
        const int t = __ffsll((long long)G) - 1;     // the tile at the head of the group; G keeps the ones behind it
        G &= G - 1;
        const uint32_t c0 = craw[0];
#pragma unroll
        for (int i = 0; i + 1 < D; i++) craw[i] = craw[i + 1];
        const int K0 = (int)(c0 & 0xFFFFu), K3 = (int)(c0 >> 16);       // ACGT matches, the pair's valid count
        const int T_used = T;
        const int base_u = (tb + t) * 64;
        const bool valid = (base_u + lane >= r_begin && base_u + lane < r_end);
        auto may_enter = [&]() -> bool { return valid && K3 - K0 < T && (!full || K0 >= W[0]); };
        unsigned long long mask = __ballot(may_enter());
        auto request = [&](int i_) -> ExtraReq {
          const int rl_ = base_u + i_;
          ExtraReq e = wave_iupac_request(db, (size_t)tile_first + (size_t)(rl_ >> 6), rl_ & 63, W4, amb + (size_t)rl_ * AMB_ROW, aq_n, aq_w, lane);
          e.nn = nonn[rl_];
          return e;
        };
        // the head of the mask and the candidate behind it are kept requested: the requests depend on the reference only, so one whose
        // candidate drops out of the mask after an admission is merely wasted
        ExtraReq nxt;
        int nxt_i = -1;
        while (mask) {
          const int i = __ffsll((long long)mask) - 1;
          const unsigned long long behind = mask & (mask - 1);
          const int i2 = behind ? (__ffsll((long long)behind) - 1) : -1;
          ExtraReq cur;
          if (nxt_i == i) { cur = nxt; nxt_i = -1; }
          else cur = request(i);
          if (i2 >= 0 && nxt_i != i2) { nxt = request(i2); nxt_i = i2; }
          const int rl = base_u + i;                                      // index relative to the first tile of the batch
          const int cx = __builtin_amdgcn_readlane(K0, i), cy = __builtin_amdgcn_readlane(K3, i);
          const size_t tile_abs = (size_t)tile_first + (size_t)(rl >> 6);
          int Si[6];
          n_demand++;
          const int4 zero = make_int4(0, 0, 0, 0);                        // no consensus counters in this regime
          const bool accept = replay_exact_default<true>(cur, db, tile_abs, rl & 63, W4, qw, qlisted, aq_n, lane, cx, cy, zero, zero, __builtin_amdgcn_readfirstlane(cur.nn), T, full, W, Si, n_dense);
          if (!accept) { mask = behind; continue; }
          replay_admit<false, true>(h, k, n, T, full, W, mc, true, Si, ord_base, r_begin, rl, entered, lane);
          dirty = true; n_admit++;
          mask = __ballot(lane > i && may_enter());
        }
        P &= ~(1ull << t);                                                // this tile is done
        if (T != T_used) {
          // Needed tiles under the new tolerance, after this one.  A lower tolerance only removes tiles: the ones in flight are
          // processed anyway (their ballots come out empty).  A higher tolerance can add a tile that lies BEFORE the last tile in
          // flight; only then is the group formed again to keep the stream order.
          P = needed() & ~((2ull << t) - 1ull);
          if (T > T_used && G && (P & ~G & ((1ull << (63 - __clzll((long long)G))) - 1ull)) != 0ull) break;
          P |= G;                                                         // keep the tiles in flight in the pending set
        }
      }
    }
  }
  replay_store_state(h, hg, n_g, T_g, q, n, T, dirty, stats, n_admit, n_demand, n_dense, lane);
}

// Replay over the packed-plane scan that also left the other two counters of every pair (scan2_extras: `ext`), default mode.
// The same machine as replay2_kernel -- one wave per query, the tile bounds walked 64 at a time, only tiles that can admit under the
// present state are opened, in stream order -- rebuilt around two facts about a handful of queries:
//   * Every lane knows its reference's whole score vector from three dwords (the two scan counters, the extras, the reference's valid
//     sites; + the packed consensus pre-score with CONS), so the ballot runs the EXACT test of src/nearest.c:488-496 + src/min_heap.c:95
//     for 64 references at once and an admission is: first set bit, six v_readlane, the heap update -- no memory round trip.
//   * The scan next to it saturates HBM, a dependent load takes microseconds, and with close sequences nearly half of the tiles pass
//     the bounds: what the wave waited for was the counters of the tiles it opened, eight tiles per round trip.  Here the counters of
//     ALL needed tiles of half a round (32 tiles) travel at once, memory -> LDS without passing registers (global_load_lds_dword: one
//     instruction moves a tile's 64 dwords), and the NEXT half round's are requested -- for the tiles the present state would open --
//     before this one is worked on.  A tile that turns out to be needed after all (the tolerance rose) is fetched when it is reached.
// A pair whose extras are unknown (an ambiguity-word list overflowed) or whose consensus pre-score was cut at the batch snapshot
// (src/nearest.c:431-432) is "slow": tested conservatively in the ballot, its counters on demand as in replay2_kernel.
// One dword per lane from memory straight into LDS (lane l's dword lands at lds_byte_addr + 4 l), no register in between and nothing
// to wait for until the data is used.  Written as inline assembly on purpose: the compiler makes every LDS read that follows a
// global_load_lds it knows of wait for ALL of them (it cannot tell the staging rows apart), which would serialise the half round being
// worked on with the one in flight.  The waits are placed by hand (replay_wait_staged); the compiler's own vmcnt waits only get
// stricter by loads it does not know of (the counter is in order).  M0 holds the LDS address: both helpers write it and declare it clobbered.
// (the compiler reserves M0 and says so for every clobber that names it; the declaration stays for the day it keeps a value there)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
static __device__ __forceinline__ void lds_dma_dword(const void *g, uint32_t lds_byte_addr)
{ asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" ::"s"(__builtin_amdgcn_readfirstlane(lds_byte_addr)), "v"(g) : "memory", "m0"); }
static __device__ __forceinline__ void lds_dma_dwordx4(const void *g, uint32_t lds_byte_addr)      // 16 bytes per lane, lane l's at lds_byte_addr + 16 l
{ asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(__builtin_amdgcn_readfirstlane(lds_byte_addr)), "v"(g) : "memory", "m0"); }
#pragma clang diagnostic pop
static __device__ __forceinline__ void replay_wait_staged() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ const uint4 g_replay_zero16 = {0u, 0u, 0u, 0u};        // what a lane past the slice's last tile stages as its bounds
typedef __attribute__((address_space(3))) void replay_lds_void;
template <bool CONS, int HALF /* tiles per staging buffer: 32, 16 or 8 -- (one CU holds 1, 3 or 4 such blocks) */>
__global__ __launch_bounds__(64) void replay3_kernel(const uint32_t *__restrict__ cnt /* ACGT matches | valid pairs << 16 */, const uint32_t *__restrict__ ext, int ppad,
                                                      const int4 *__restrict__ rt, const uint32_t *__restrict__ rtp /* CONS: rt.x | (rt.w - rt.x) << 16 */, const uint32_t *__restrict__ cp_cons,
                                                      const int *__restrict__ nonn, const int *__restrict__ amb,
                                                      int r_begin, int r_end, long long ord_base, int *__restrict__ heap_g, int *__restrict__ n_g, int *__restrict__ T_g,
                                                      const int *__restrict__ snap_ptr, uint8_t *__restrict__ entered, int k, const uint4 *__restrict__ db, long long tile_first, int W4,
                                                      const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q, unsigned long long *__restrict__ stats, int q_first,
                                                      const uint4 *__restrict__ tb8 /* per (query, tile): tile_bounds8 */, int prio_)
{
  extern __shared__ int h[];
  constexpr int NA = CONS ? 4 : 3, NSUB = 64 / HALF;           // arrays staged per tile; staging-buffer fills per round of 64 tiles
  constexpr unsigned long long SUB0 = HALF == 32 ? 0xFFFFFFFFull : HALF == 16 ? 0xFFFFull : 0xFFull;
  static_assert(HALF == 32 || HALF == 16 || HALF == 8, "staging buffers of 32, 16 or 8 tiles");
#ifdef REPLAY_TIMING
  const unsigned long long tt_kernel = wall_clock64();
#endif
  if (prio_) __builtin_amdgcn_s_setprio(3);
  const int q = blockIdx.x + q_first, lane = threadIdx.x;
  int *hg = heap_g + (size_t)q * (k + 1) * HEAP_ENTRY;
  int n = replay_load_heap(h, hg, n_g[q], k, lane), T = T_g[q];     // (no barrier of its own: replay_query_listed's first one publishes the heap)
  const int snap = *snap_ptr;
  const uint32_t *crow = cnt + (size_t)q * ppad, *xrow = ext + (size_t)q * ppad;
  const uint32_t *qrow = qfull + (size_t)q * W4 * 4 * 6;
  uint32_t *qlisted = reinterpret_cast<uint32_t *>(h + (k + 1) * HEAP_ENTRY);           // bitmap of the words the query lists (slow pairs)
  constexpr int BR = 16;                                                                // rounds of bounds the LDS ring holds
  uint4 *bring = reinterpret_cast<uint4 *>(qlisted + 32);                               // [BR][64] uint4: the bounds of round x in slot x & 15
  uint32_t *stage = reinterpret_cast<uint32_t *>(bring + BR * 64);                      // [2][HALF][NA][64] dwords
  const uint32_t stage_lds = (uint32_t)(uintptr_t)(replay_lds_void *)stage, bring_lds = (uint32_t)(uintptr_t)(replay_lds_void *)bring;
  int aq_n, aq_w;
  replay_query_listed<false>(amb_q, q, lane, qlisted, aq_n, aq_w);
  bool full;
  int W[6], mc;
  const bool use_mc = replay_heap_state<false>(h, n, k, lane, full, W, mc);
  bool dirty = false;
  unsigned n_admit = 0, n_demand = 0, n_dense = 0, n_open = 0;
#ifdef REPLAY_TIMING
  unsigned long long tt_wait = 0, tt_fetch = 0, tt_admit = 0, tt_tile = 0, tt_late = 0, n_late = 0; const unsigned long long tt_begin = tt_kernel, tt_prologue_end = wall_clock64();
#endif
  const uint4 *tmrow = tb8 + (size_t)q * (ppad >> 6);
  const int n_slice_tiles = (r_end + 63) >> 6, n_rounds = (n_slice_tiles + 63) >> 6;
  // The bounds travel memory -> LDS as well, rounds ahead and without a register to wait for: the bounds of round x sit in slot x & 15
  // of a ring, requested in groups of four rounds at least two rounds before their first use; the wave waits once per group.
  auto fetch_bounds = [&](int r) {
    if (r >= n_rounds) return;
    const int t = r * 64 + lane;
    const uint4 *src = t < n_slice_tiles ? tmrow + t : &g_replay_zero16;
    lds_dma_dwordx4(src, bring_lds + (uint32_t)(r & (BR - 1)) * 1024u);
  };
  // the counters of tile `t` (slice numbering) into row (t & 31) of staging buffer b: one instruction per array, 256 B each
  auto fetch_tile = [&](int t, int b) {
    const uint32_t row = stage_lds + (uint32_t)((b * HALF + (t & (HALF - 1))) * NA) * 256u;
    const size_t r = (size_t)t * 64 + lane;
    lds_dma_dword(crow + r, row);
    lds_dma_dword(xrow + r, row + 256u);
    lds_dma_dword(nonn + r, row + 512u);
    if (CONS) lds_dma_dword(rtp + r, row + 768u);
  };
  auto fetch_tiles = [&](unsigned long long m, int tb, int b) { for (; m; m &= m - 1) fetch_tile(tb + __ffsll((long long)m) - 1, b); };
  // A tile can admit only if one of its references passes the gate and (heap full) reaches the worst kept first key: the tile's entry
  // for the smallest threshold >= T - 1 is 1 + the largest first key among the references with at most that many mismatches (0: none).
  // With CONS a cut pre-score lowers a pair's mismatch count, but never below the snapshot: once T exceeds it, any count may pass.
  auto needed = [&](const uint4 &tb_) -> unsigned long long {
    int j = TB8_N - 1;
    if (!(CONS && snap < T)) {
#pragma unroll
      for (int i = TB8_N - 2; i >= 0; i--) if (TB8_THR[i] >= T - 1) j = i;
    }
    const uint32_t w = (j >> 1) == 0 ? tb_.x : (j >> 1) == 1 ? tb_.y : (j >> 1) == 2 ? tb_.z : tb_.w;       // (j is wave-uniform)
    const uint32_t e = (j & 1) ? (w >> 16) : (w & 0xFFFFu);
    return __ballot(e != 0u && (!full || (int)e > W[0]));
  };
  unsigned long long have[2] = {0ull, 0ull};                  // tiles (bits of their round) whose counters are in, or on their way to, each staging buffer
  for (int r = 0; r < 9; r++) fetch_bounds(r);
  replay_wait_staged();
  have[0] = needed(bring[lane]) & SUB0;
  fetch_tiles(have[0], 0, 0);
  for (int rnd = 0; rnd < n_rounds; rnd++) {
    const int tb = rnd * 64;
    bool waited = false;
    if ((rnd & 3) == 3) {                                     // the bounds of rounds rnd + 1 .. rnd + 5 have arrived (requested >= 3 rounds ago); the next group
      TT_START(t_); replay_wait_staged(); TT_ADD(tt_wait, t_);
      for (int r = rnd + 6; r < rnd + 10; r++) fetch_bounds(r);
      waited = true;
    }
    const uint4 tbv = bring[(rnd & (BR - 1)) * 64 + lane];    // bounds of this round's tiles
#pragma unroll 1
    for (int hb = 0; hb < NSUB; hb++) {                       // the round's parts: tiles tb + HALF hb .. + HALF - 1, staged in buffer hb & 1
      const int b = hb & 1;
      const unsigned long long half_mask = SUB0 << (HALF * hb);
      if (have[b] && !waited) { TT_START(t_); replay_wait_staged(); TT_ADD(tt_wait, t_); }   // this half's counters are in LDS (requested one half ago)
      waited = false;
      TT_START(tf_);
      // the next half's counters, for the tiles the present state would open
      if (hb + 1 < NSUB) { have[b ^ 1] = needed(tbv) & (SUB0 << (HALF * (hb + 1))); fetch_tiles(have[b ^ 1], tb, b ^ 1); }
      else if (rnd + 1 < n_rounds) { have[0] = needed(bring[((rnd + 1) & (BR - 1)) * 64 + lane]) & SUB0; fetch_tiles(have[0], tb + 64, 0); }
      TT_ADD(tt_fetch, tf_);
      unsigned long long P = needed(tbv) & half_mask;
      while (P) {
        TT_START(tt0_);
        const int tsel = __ffsll((long long)P) - 1;
        P &= P - 1;
        if (!((have[b] >> tsel) & 1ull)) {                   // needed after all (the tolerance rose since the half was requested)
          TT_START(tl_);
          fetch_tile(tb + tsel, b);
          have[b] |= 1ull << tsel;
          replay_wait_staged();
          TT_ADD(tt_late, tl_);
#ifdef REPLAY_TIMING
          n_late++;
#endif
        }
        n_open++;
        const uint32_t *row = stage + (size_t)((b * HALF + (tsel & (HALF - 1))) * NA) * 64 + lane;
        const uint32_t craw = row[0], xraw = row[64];
        const int nn = (int)row[128];
        const uint32_t araw = CONS ? row[192] : 0u;
        const int base_u = (tb + tsel) * 64;
        const bool valid = (base_u + lane >= r_begin) && (base_u + lane < r_end);
        const int K0 = (int)(craw & 0xFFFFu), V = (int)(craw >> 16);
        const int ax = (int)(araw & 0xFFFFu), mc_true = (int)(araw >> 16);
        const bool cut = CONS && mc_true >= snap;
        const bool slow = cut || xraw == EXT_UNKNOWN;
        // score[] as src/nearest.c:499-501 assembles it (a pair that is not cut: its own counters)
        int S[6];
        S[0] = K0; S[1] = K0 + (int)(xraw & 0xFFFFu); S[2] = S[1] + (int)(xraw >> 16); S[3] = V; S[4] = K0 - ax; S[5] = nn;
        const int m = V - K0 - (cut ? mc_true - snap : 0);
        auto may_enter = [&]() -> bool {
          if (!valid || m >= T) return false;
          if (!full) return true;
          if (slow) return K0 >= W[0];                        // keys of a slow pair: upper bounds until its counters are known
          return lex_better(S, W);
        };
        unsigned long long mask = __ballot(may_enter());
        if (!mask) { TT_ADD(tt_tile, tt0_); continue; }
        TT_START(ta_);
        const unsigned long long slow_mask = __ballot(slow), cut_mask = __ballot(cut);
        const int T_used = T;
        bool admitted_here = false;
        while (mask) {
          const int i = __ffsll((long long)mask) - 1;
          const int rl = base_u + i;
          int Si[6];
          if ((slow_mask >> i) & 1ull) {                      // wave-uniform
            const size_t tile_abs = (size_t)tile_first + (size_t)(rl >> 6);
            const int cx = __builtin_amdgcn_readlane(K0, i), cy = __builtin_amdgcn_readlane(V, i);
            int4 ai = make_int4(0, 0, 0, 0);
            if (CONS) ai = rt[rl];
            int4 ri = ai;
            if (CONS && ((cut_mask >> i) & 1ull)) ri = wave_truncated_consensus<false>(db, tile_abs, rl & 63, W4, cp_cons, snap, lane);
            n_demand++;
            const ExtraReq cur = wave_iupac_request(db, tile_abs, rl & 63, W4, amb + (size_t)rl * AMB_ROW, aq_n, aq_w, lane);
            const bool accept = replay_exact_default<false>(cur, db, tile_abs, rl & 63, W4, qrow, qlisted, aq_n, lane, cx, cy, ai, ri, __builtin_amdgcn_readlane(nn, i), T, full, W, Si, n_dense);
            if (!accept) { mask &= mask - 1; continue; }
          } else {                                            // the ballot ran the exact test under the present state
#pragma unroll
            for (int s_ = 0; s_ < 6; s_++) Si[s_] = __builtin_amdgcn_readlane(S[s_], i);
          }
          replay_admit<false, false>(h, k, n, T, full, W, mc, use_mc, Si, ord_base, r_begin, rl, entered, lane);
          dirty = true; n_admit++; admitted_here = true;
          mask = __ballot(lane > i && may_enter());
        }
        // the tiles still to open in this half under the new state, after this one: a higher worst key only removes tiles, a higher
        // tolerance can add some -- all of them lie ahead (tiles are opened strictly in stream order)
        if (admitted_here || T != T_used) P = needed(tbv) & half_mask & ~((2ull << tsel) - 1ull);
        TT_ADD(tt_admit, ta_);
        TT_ADD(tt_tile, tt0_);
      }
    }
  }
  replay_wait_staged();                                       // nothing of this wave is in flight to its LDS when it ends
#ifdef REPLAY_TIMING
  if (lane == 0) { atomicAdd(&stats[4], tt_wait); atomicAdd(&stats[5], tt_fetch); atomicAdd(&stats[6], tt_tile); atomicAdd(&stats[7], tt_admit); atomicAdd(&stats[8], tt_late); atomicAdd(&stats[9], n_late); atomicAdd(&stats[10], wall_clock64() - tt_begin);
                   atomicAdd(&stats[11], tt_prologue_end - tt_kernel); atomicAdd(&stats[12], 1ull); }
#endif
  replay_store_state(h, hg, n_g, T_g, q, n, T, dirty, stats, n_admit, n_demand, n_dense, lane);
  if (stats && lane == 0) atomicAdd(&stats[3], (unsigned long long)n_open);
}

// Redundancy test of exclude_redundant_query_sequences() (src/fastaseq.c:806-808): a sequence and a query "agree" when the
// truncated distance on the polymorphic columns (maxdist 1, src/fastaseq.c:562-583) is zero.  out[r * nq + q], one byte.
template <bool ACGT>
__global__ void agree_kernel(const int4 *__restrict__ cnt_q, int ppad, int nq, int n_ref, uint8_t *__restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (r >= n_ref) return;
  const int4 c = cnt_q[(size_t)q * ppad + r];
  out[(size_t)r * nq + q] = (uint8_t)((ACGT ? c.x : (c.w - c.y)) == 0);
}

__global__ void snapshot_kernel(const int *__restrict__ T, int nq, int *__restrict__ snap)
{ // cq->max_incompatible = max over heaps (src/nearest.c:290-291)
  __shared__ int red[256];
  int v = -0x7fffffff;
  for (int i = threadIdx.x; i < nq; i += 256) v = max(v, T[i]);
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]); __syncthreads(); }
  if (threadIdx.x == 0) *snap = red[0];
}

// uvaia_gpu_reset in one launch (grid-stride): empty heaps, T = nchar and n = 0 for every query (src/nearest.c:375,387 ; src/min_heap.c:56),
// the batch snapshot = nchar (cq->max_incompatible = n_sites, src/nearest.c:375) and the entered flags of the resident database cleared.
// heap16 / entered16: length of the two arrays in units of 16 bytes (both are whole multiples: a heap entry is 32 bytes, the flags come in
// tiles of 64).
__global__ __launch_bounds__(256)
void reset_state_kernel(uint4 *__restrict__ heap, size_t heap16, int *__restrict__ T, int *__restrict__ n, int nq, int nchar,
                        int *__restrict__ snap, uint4 *__restrict__ entered, size_t entered16)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (size_t i = i0; i < heap16; i += stride) heap[i] = z;
  for (size_t i = i0; i < entered16; i += stride) entered[i] = z;
  for (size_t i = i0; i < (size_t)nq; i += stride) { T[i] = nchar; n[i] = 0; }
  if (i0 == 0) *snap = nchar;
}

// untruncated score vectors of a batch, for parity tests: out[(i*nq+q)*6+s]
template <bool ACGT>
__global__ void batch_scores_kernel(const int4 *__restrict__ cnt, int ppad, const int4 *__restrict__ rt, const int *__restrict__ nonn,
                                    int r_begin, int n_ref, int nq, int *__restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (i >= n_ref) return;
  const int r = r_begin + i;
  int S[6], m;
  assemble_scores<ACGT>(cnt[(size_t)q * ppad + r], rt[r], rt[r], nonn[r], S, m);
  for (int s = 0; s < 6; s++) out[((size_t)i * nq + q) * 6 + s] = S[s];
}
