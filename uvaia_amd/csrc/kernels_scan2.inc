// kernels_scan2.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the four-counter scans scan_iupac_kernel / scan_acgt_kernel (introspection, radius search, query pruning, alignments above 49 000 columns), the two-counter scans over the packed planes scan2_iupac_kernel / scan2_acgt_kernel (what up to 16 queries run: one query tile, every reference byte read once, nothing derived), pair_extras_kernel and tile_bounds_kernel (the other two counters of every pair and the sharp tile bounds, behind the column-compressed scan), and the device helpers the scans share (load_qwords, scan_work_item, wave_max_dpp).

// ------------------------------------------------------------------------------------------------------------
// device: the four-counter pair scan
// ------------------------------------------------------------------------------------------------------------
template <int N> struct QWords { uint32_t v[N]; };
template <int N, typename PTR> static __device__ __forceinline__ void load_qwords(QWords<N> &d, PTR p)
{
#pragma unroll
  for (int i = 0; i < N; i++) d.v[i] = p[i];   // wave-uniform address -> s_load_dwordx8/x16
}
// (Scalar loads return out of order: the only wait for them is lgkmcnt(0), for all that are outstanding.  In the loops below the compiler's
// wait for the present query's words therefore lands behind the request for the next one and covers both -- the unrolled loop pays one
// scalar-load latency per TWO queries.  Pinning the wait in front of the request (one latency per query, each partly covered by the
// arithmetic of one query) is much slower, round 4: 16 queries x 1 M references 7.1 ms per step against 4.2, 32 queries 12.2 against
// 7.1, config[1] 3.07 against 3.00 -- next to a scan that streams the packed planes a scalar load takes about a microsecond.)
// Default mode: 4 planes (A,C,G,T bits of the IUPAC set).  Per (reference, query) pair and 32-site word:
//   r0 = #(equal & ACGT)  r1 = #(equal & both valid)  r2 = #(sets intersect)  r3 = #(both valid)
// (the four counters of the biomcmc kernel, call sites src/nearest.c:491,495).  15 VALU ops per pair-word.
// query planes per word: A,C,G,T, valid, is-ACGT.
template <int QT>
__global__ __launch_bounds__(256) void scan_iupac_kernel(const uint4 *__restrict__ db, long long tile_first, int n_tiles, int W4,
                                                          const uint32_t *__restrict__ qp, int4 *__restrict__ out, int ppad)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int trel = blockIdx.y * 4 + wave;
  if (trel >= n_tiles) return;
  const int q0 = blockIdx.x * QT;
  int acc[QT][4];
#pragma unroll
  for (int q = 0; q < QT; q++) { acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0; }
  const uint4 *t = db + (size_t)(tile_first + trel) * W4 * 4 * 64 + lane;
  const size_t qstride = (size_t)W4 * 24;
  const uint32_t *qb = qp + (size_t)q0 * qstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    const uint32_t rA[4] = {pA.x, pA.y, pA.z, pA.w}, rC[4] = {pC.x, pC.y, pC.z, pC.w}, rG[4] = {pG.x, pG.y, pG.z, pG.w}, rT[4] = {pT.x, pT.y, pT.z, pT.w};
    uint32_t rv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) rv[j] = rA[j] | rC[j] | rG[j] | rT[j];
    const uint32_t *s0 = qb + (size_t)w4 * 24;
    QWords<24> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int q = 0; q < QT; q++) {
      if (q + 1 < QT) load_qwords(nxt, s0 + (size_t)(q + 1) * qstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t qA = cur.v[j * 6 + 0], qC = cur.v[j * 6 + 1], qG = cur.v[j * 6 + 2], qT_ = cur.v[j * 6 + 3], qv = cur.v[j * 6 + 4], qa = cur.v[j * 6 + 5];
        uint32_t d = rA[j] ^ qA;
        d = B3(rC[j], qC, d, (TT_A ^ TT_B) | TT_C);
        d = B3(rG[j], qG, d, (TT_A ^ TT_B) | TT_C);
        const uint32_t nd = B3(rT[j], qT_, d, ~((TT_A ^ TT_B) | TT_C));   // all four planes equal
        uint32_t x = rA[j] & qA;
        x = B3(rC[j], qC, x, (TT_A & TT_B) | TT_C);
        x = B3(rG[j], qG, x, (TT_A & TT_B) | TT_C);
        x = B3(rT[j], qT_, x, (TT_A & TT_B) | TT_C);                       // sets intersect (implies both valid)
        acc[q][0] = bcnt_acc(nd & qa, acc[q][0]);
        acc[q][1] = bcnt_acc(nd & rv[j], acc[q][1]);
        acc[q][2] = bcnt_acc(x, acc[q][2]);
        acc[q][3] = bcnt_acc(rv[j] & qv, acc[q][3]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (q + 1 < QT) cur = nxt;
    }
  }
  const size_t r = (size_t)trel * 64 + lane;
#pragma unroll
  for (int q = 0; q < QT; q++) out[(size_t)(q0 + q) * ppad + r] = make_int4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
}

// --acgt mode: 3 planes (lo, hi of the 2-bit code, is-ACGT).  Per pair-word:
//   c0 = #(both ACGT & differ)  c1 = #(both ACGT)  c2 = #(both ACGT & differ) on polymorphic query columns
// (src/fastaseq.c:585-596; c2 separates score[5] from score[4], src/nearest.c:468-469).  8 VALU ops per pair-word.
// query planes per word: lo, hi, is-ACGT, is-ACGT restricted to the polymorphic columns (query->idx).
template <int QT>
__global__ __launch_bounds__(256) void scan_acgt_kernel(const uint4 *__restrict__ db, long long tile_first, int n_tiles, int W4,
                                                         const uint32_t *__restrict__ qp, int4 *__restrict__ out, int ppad)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int trel = blockIdx.y * 4 + wave;
  if (trel >= n_tiles) return;
  const int q0 = blockIdx.x * QT;
  int acc[QT][3];
#pragma unroll
  for (int q = 0; q < QT; q++) { acc[q][0] = acc[q][1] = acc[q][2] = 0; }
  const uint4 *t = db + (size_t)(tile_first + trel) * W4 * 3 * 64 + lane;
  const size_t qstride = (size_t)W4 * 16;
  const uint32_t *qb = qp + (size_t)q0 * qstride;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pL = t[(size_t)(w4 * 3 + 0) * 64], pH = t[(size_t)(w4 * 3 + 1) * 64], pI = t[(size_t)(w4 * 3 + 2) * 64];
    const uint32_t rL[4] = {pL.x, pL.y, pL.z, pL.w}, rH[4] = {pH.x, pH.y, pH.z, pH.w}, rI[4] = {pI.x, pI.y, pI.z, pI.w};
    const uint32_t *s0 = qb + (size_t)w4 * 16;
    QWords<16> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int q = 0; q < QT; q++) {
      if (q + 1 < QT) load_qwords(nxt, s0 + (size_t)(q + 1) * qstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t qL = cur.v[j * 4 + 0], qH = cur.v[j * 4 + 1], qI = cur.v[j * 4 + 2], qIp = cur.v[j * 4 + 3];
        const uint32_t d = rL[j] ^ qL;
        const uint32_t y = B3(rH[j], qH, d, (TT_A ^ TT_B) | TT_C);     // codes differ
        acc[q][0] = bcnt_acc(B3(y, rI[j], qI, TT_A & TT_B & TT_C), acc[q][0]);
        acc[q][1] = bcnt_acc(rI[j] & qI, acc[q][1]);
        acc[q][2] = bcnt_acc(B3(y, rI[j], qIp, TT_A & TT_B & TT_C), acc[q][2]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (q + 1 < QT) cur = nxt;
    }
  }
  const size_t r = (size_t)trel * 64 + lane;
#pragma unroll
  for (int q = 0; q < QT; q++) out[(size_t)(q0 + q) * ppad + r] = make_int4(acc[q][0], acc[q][1], acc[q][2], 0);
}

// XCD-aware work mapping for the scans (1-D grid).  Blocks are dealt round-robin over the 8 XCDs (each with its own L2), so
// block b runs on XCD b % 8.  All query tiles of one reference group are given ids with the same b % 8: the group's tiles
// are then fetched by ONE L2 instead of eight, and consecutive slots of an XCD share the group (temporal locality).
// Placement only affects speed/traffic, never results.
static __device__ __forceinline__ bool scan_work_item(int n_qtiles, int n_groups, int &qtile, int &group)
{
  const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
  qtile = slot % n_qtiles;
  group = (slot / n_qtiles) * 8 + xcd;
  return group < n_groups;
}
static inline unsigned scan_grid_size(int n_qtiles, int n_groups) { return (unsigned)n_qtiles * (unsigned)((n_groups + 7) / 8) * 8u; }

// ------------------------------------------------------------------------------------------------------------
// device: the two-counter pair scan over the packed planes (production path for at most 16 queries)
// ------------------------------------------------------------------------------------------------------------
// The gate of src/nearest.c:488-496 only needs the mismatch count m = valid - ACGT_matches of a pair, and the heap
// order is decided by ACGT_matches first (src/min_heap.c:41-47).  The dense pass therefore counts just
//   default: r0 = #(equal & ACGT), r3 = #(both valid)          --acgt: c0 = #(both ACGT & differ), c1 = #(both ACGT)
// and the replay kernel fetches the remaining counters of the few pairs that reach the heap (below).
// Reference words are re-coded per word into (lo, hi, isACGT, valid); query planes arrive in that coding.
// Per (query, tile of 64 references): {smallest mismatch count, largest ACGT-match count} over the references of the batch, the
// two bounds the replay skips tiles by (same definition as scan3_kernel's epilogue).
// Sharper bounds for the replay of a handful of queries (replay3_kernel).  A tile can admit something only if ONE reference both passes
// the gate (mismatches < tolerance) and reaches the worst kept first key; the two separate bounds above say "some reference does the
// one, some reference the other", which with close sequences is true of nearly half of all tiles although a few in ten thousand
// references enter a heap -- and every opened tile costs the lone replay wave a few hundred nanoseconds.  Per (query, tile) eight
// 16-bit entries instead: entry j = 1 + the largest ACGT-match count among the tile's references (of the batch) with at most
// TB8_THR[j] mismatches, 0 if there is none (the last entry: any number of mismatches).  The replay reads the entry of the smallest
// threshold >= tolerance - 1: exact up to the threshold's granularity, for any sequence of tolerances.
constexpr int TB8_N = 8;
__device__ constexpr int TB8_THR[TB8_N - 1] = {0, 1, 2, 3, 5, 8, 14};
static __device__ __forceinline__ uint32_t wave_max_dpp(uint32_t v)
{ // maximum over the wave by DPP (row shifts, then row broadcasts; lanes without a source see 0); result from lane 63
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
static __device__ __forceinline__ uint4 tile_bounds8(int mm, int kk, bool in_batch)
{
  uint32_t e[TB8_N];
#pragma unroll
  for (int j = 0; j < TB8_N; j++) e[j] = wave_max_dpp((in_batch && (j == TB8_N - 1 || mm <= TB8_THR[j])) ? (uint32_t)(kk + 1) : 0u);
  return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// the four waves' partial counts of a tile summed in LDS; wave v then writes queries v, v + 4, ...: the pair counters and the two
// bounds of the (query, tile) (same definition as scan3_kernel's epilogue); wave 0 also the consensus pre-score
template <int QT, bool ACGT, bool CONS>
static __device__ __forceinline__ void scan2_finish(int (&red)[2 * QT + 4][64], const int (&acc)[QT][2], int cc0, int cc1, int cc2, int cc3,
                                                    uint32_t *__restrict__ out, int ppad, const int *__restrict__ tot, int2 *__restrict__ tmin, int r_lo, int r_hi,
                                                    int4 *__restrict__ rt, int q0, int qtile, int trel, int lane, int wave, uint32_t *__restrict__ rtp = nullptr,
                                                    uint4 *__restrict__ tb8 = nullptr /* default mode: the eight-entry bounds instead of tmin */)
{
  // the four waves' partial counts meet in ONE array of LDS counters (adds; a copy per wave -- 37 KB at 16 queries -- held a CU to four
  // blocks, i.e. four waves per SIMD, too few to cover the plane loads of a kernel that is meant to run at HBM speed)
  for (int i = threadIdx.x; i < (2 * QT + 4) * 64; i += 256) (&red[0][0])[i] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < QT; q++) { atomicAdd(&red[2 * q][lane], acc[q][0]); atomicAdd(&red[2 * q + 1][lane], acc[q][1]); }
  if (CONS) { atomicAdd(&red[2 * QT][lane], cc0); atomicAdd(&red[2 * QT + 1][lane], cc1); atomicAdd(&red[2 * QT + 2][lane], cc2); atomicAdd(&red[2 * QT + 3][lane], cc3); }
  __syncthreads();
  auto sum4 = [&](int k) { return red[k][lane]; };
  const int r = trel * 64 + lane;
  const int total = tot[r];
  const bool in_batch = (r >= r_lo && r < r_hi);
  for (int q = wave; q < QT; q += 4) {
    const int c0 = sum4(2 * q), c1 = total - sum4(2 * q + 1);
    out[(size_t)(q0 + q) * ppad + r] = (uint32_t)c0 | ((uint32_t)c1 << 16);
    if (!ACGT && tb8) {
      const uint4 b8 = tile_bounds8(c1 - c0, c0, in_batch);
      if (lane == 0) tb8[(size_t)(q0 + q) * (ppad >> 6) + trel] = b8;
    } else if (tmin) {
      const int mm = ACGT ? c0 : c1 - c0, kk = ACGT ? c1 - c0 : c0;
      int m = in_batch ? mm : 0x7fffffff, k = in_batch ? kk : (int)0x80000000;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { m = min(m, __shfl_xor(m, o)); k = max(k, __shfl_xor(k, o)); }
      if (lane == 0) tmin[(size_t)(q0 + q) * (ppad >> 6) + trel] = make_int2(m, k);
    }
  }
  if (CONS && qtile == 0 && wave == 0) {
    rt[r] = make_int4(sum4(2 * QT), sum4(2 * QT + 1), sum4(2 * QT + 2), sum4(2 * QT + 3));
    // what replay3_kernel needs of it per lane, in one dword: ACGT matches with the consensus | its mismatches << 16 (default mode; both below 2^16)
    if (rtp) rtp[r] = (uint32_t)sum4(2 * QT) | ((uint32_t)(sum4(2 * QT + 3) - sum4(2 * QT)) << 16);
  }
}

// contribution of one alignment word to  d1 = #(equal & valid & not ACGT) = text_matches - ACGT_matches  and
// d2 = #(sets intersect & not equal) = partial_matches - text_matches  of a pair, given both sets of four IUPAC planes and the
// query's "is ACGT" word (the two counters the two-counter scans leave out; biomcmc's kernel, call sites src/nearest.c:491,495)
static __device__ __forceinline__ void iupac_planes_extra(uint32_t rA, uint32_t rC, uint32_t rG, uint32_t rT, uint32_t qA, uint32_t qC, uint32_t qG, uint32_t qT_,
                                                          uint32_t qa, int &d1, int &d2)
{
  const uint32_t rv = rA | rC | rG | rT;
  const uint32_t nd = ~((rA ^ qA) | (rC ^ qC) | (rG ^ qG) | (rT ^ qT_));
  const uint32_t e = nd & rv, a0 = nd & qa, x = (rA & qA) | (rC & qC) | (rG & qG) | (rT & qT_);
  d1 += __popc(e & ~a0);
  d2 += __popc(x & ~e);
}

// The two counters the packed-plane scan does not count -- text_matches - ACGT_matches and partial_matches - text_matches -- for EVERY
// pair of the tile, so that the ordered replay needs no round trip to memory per admission (with a handful of queries the replays are
// the step and an admission was one dependent fetch, DESIGN.md 4.4).  Both differences live on alignment words where the reference or
// the query carries a partially ambiguous code: the reference's words come with their planes in its side row (lane = reference: a
// loop of as many trips as the tile's longest list, 1.7 words on average), the query's words are wave-uniform.  Exact; a pair whose
// lists are incomplete (more than AMB_CAP words) gets EXT_UNKNOWN and the replay counts it on demand as before.
//   ext[q][r] = d1 | d2 << 16.   Wave v of the block takes queries v, v + 4, ... of the tile (as scan2_finish does).
constexpr uint32_t EXT_UNKNOWN = 0xFFFFFFFFu;
template <int QT>
static __device__ __forceinline__ void scan2_extras(const uint4 *__restrict__ db, long long tile_abs, int trel, int W4, const int *__restrict__ amb,
                                                    const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q, int q0, int nq,
                                                    uint32_t *__restrict__ ext, int ppad, int lane, int wave)
{
  constexpr int QW = (QT + 3) / 4;
  const uint32_t *dbw = reinterpret_cast<const uint32_t *>(db);
  const int *row = amb + ((size_t)tile_abs * 64 + lane) * AMB_ROW;
  const int nr = row[0];
  const bool r_known = nr <= AMB_CAP;
  int d1[QW], d2[QW], aqn[QW];
#pragma unroll
  for (int i = 0; i < QW; i++) {
    d1[i] = d2[i] = 0;
    const int q = q0 + wave + 4 * i;
    aqn[i] = (wave + 4 * i < QT && q < nq) ? __builtin_amdgcn_readfirstlane(amb_q[(size_t)q * AMB_STRIDE]) : -1;     // -1: no such query
  }
  // the words the reference lists (skipping, per query, the ones the query lists itself: those are counted below)
  int kmax = r_known ? nr : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
  for (int k = 0; k < kmax; k++) {
    const bool have = r_known && k < nr;
    const int w = have ? row[1 + k] : 0;
    int4 pl = make_int4(0, 0, 0, 0);
    if (have) pl = *reinterpret_cast<const int4 *>(row + 12 + 4 * k);
#pragma unroll
    for (int i = 0; i < QW; i++) {
      if (aqn[i] < 0 || aqn[i] > AMB_CAP) continue;                    // wave-uniform
      const int q = q0 + wave + 4 * i;
      bool listed = false;
      for (int j = 0; j < aqn[i]; j++) listed |= (w == amb_q[(size_t)q * AMB_STRIDE + 1 + j]);
      if (have && !listed) {
        const uint32_t *sq = qfull + ((size_t)q * W4 * 4 + w) * 6;
        iupac_planes_extra((uint32_t)pl.x, (uint32_t)pl.y, (uint32_t)pl.z, (uint32_t)pl.w, sq[0], sq[1], sq[2], sq[3], sq[5], d1[i], d2[i]);
      }
    }
  }
  // the words the queries list: the reference's planes from its tile, the query's words by scalar loads
#pragma unroll
  for (int i = 0; i < QW; i++) {
    if (aqn[i] < 0 || aqn[i] > AMB_CAP) continue;
    const int q = q0 + wave + 4 * i;
    for (int j = 0; j < aqn[i]; j++) {
      const int w = __builtin_amdgcn_readfirstlane(amb_q[(size_t)q * AMB_STRIDE + 1 + j]);
      const size_t base = (((size_t)tile_abs * W4 + (w >> 2)) * 4) * 256 + (size_t)lane * 4 + (w & 3);
      const uint32_t *sq = qfull + ((size_t)q * W4 * 4 + w) * 6;
      iupac_planes_extra(dbw[base], dbw[base + 256], dbw[base + 512], dbw[base + 768], sq[0], sq[1], sq[2], sq[3], sq[5], d1[i], d2[i]);
    }
  }
  const size_t r = (size_t)trel * 64 + lane;
#pragma unroll
  for (int i = 0; i < QW; i++) {
    if (aqn[i] < 0) continue;
    const int q = q0 + wave + 4 * i;
    ext[(size_t)q * ppad + r] = (r_known && aqn[i] <= AMB_CAP) ? ((uint32_t)d1[i] | ((uint32_t)d2[i] << 16)) : EXT_UNKNOWN;
  }
}

// The same two arrays for the COLUMN-COMPRESSED scan (33-128 queries, default mode; round 4): scan3_kernel reads derived planes, not the packed
// ones, so the other two counters of every pair and the eight-entry bounds come from two kernels of their own that follow it on its stream.
// There the replays -- 64 waves with a memory round trip per admission -- were the step (64 queries x 1 M references: 5 ms of back-to-back
// replay kernels next to 2 ms of scans); with both arrays the slice goes through replay3_kernel.
//   pair_extras_kernel: one block = one tile of 64 references x 16 queries; wave v takes queries v, v + 4, ... (scan2_extras).  Its cost
//     is the words the QUERIES list: four plane loads of 1 KB per (query, word, tile), of which a quarter is used -- with 64 queries of 1.5
//     listed words each 40 % of the packed bytes of the database again (0.5-0.8 ms per 166 000 references).  Measured alternatives, all
//     slower or useless: lane = query with the sums transposed through LDS, on the scan's stream or one of its own (8.9 / 8.5 ms per step
//     of 64 queries x 1 M references against 8.15); only the (query, tile) pairs whose largest first key beats the heap's worst kept one
//     (the only bound that cannot be undone by a tolerance that rises later): with sequences this close that keeps nearly every pair.
//   tile_bounds_kernel: reads the pair counters (first | second << 16) once and reduces the bounds; wave (block, v) takes tile `block`,
//     queries v, v + 4, ...; also packs the consensus pre-score (consensus_rt_kernel's) for the replay.
__global__ __launch_bounds__(256) void pair_extras_kernel(const uint4 *__restrict__ db, long long tile_first, int n_tiles, int W4, const int *__restrict__ amb,
                                                          const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q, int nq, uint32_t *__restrict__ ext, int ppad)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int trel = blockIdx.x, q0 = blockIdx.y * 16;
  if (trel >= n_tiles) return;
  scan2_extras<16>(db, tile_first + trel, trel, W4, amb, qfull, amb_q, q0, nq, ext, ppad, lane, wave);
}
__global__ __launch_bounds__(256) void tile_bounds_kernel(const uint32_t *__restrict__ cnt, int ppad, int n_tiles, int nq, int r_lo, int r_hi, uint4 *__restrict__ tb8,
                                                          const int4 *__restrict__ rt /* nullable */, uint32_t *__restrict__ rtp)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int trel = blockIdx.x;
  if (trel >= n_tiles) return;
  const int r = trel * 64 + lane;
  const bool in_batch = (r >= r_lo && r < r_hi);
  for (int q = wave; q < nq; q += 4) {
    const uint32_t c = cnt[(size_t)q * ppad + r];
    const int c0 = (int)(c & 0xFFFFu), c1 = (int)(c >> 16);
    const uint4 b8 = tile_bounds8(c1 - c0, c0, in_batch);
    if (lane == 0) tb8[(size_t)q * (ppad >> 6) + trel] = b8;
  }
  if (rt && wave == 0) { const int4 a = rt[r]; rtp[r] = (uint32_t)a.x | ((uint32_t)(a.w - a.x) << 16); }
}

// 4 logic ops + 2 v_bcnt per pair-word.
// CONS: the query set has constant-and-complete columns (query->idx_c): the untruncated consensus pre-score of every reference
// (queue_distance_to_consensus, src/nearest.c:428-433, without its early exit: kernels_consensus.inc) rides along -- the planes are
// in registers anyway, so a search of few queries reads every reference byte exactly once.
template <int QT, bool CONS>
__global__ __launch_bounds__(256) void scan2_iupac_kernel(const uint4 *__restrict__ db, long long tile_first, int n_tiles, int W4,
                                                           const uint32_t *__restrict__ qp2, uint32_t *__restrict__ out, int ppad, int n_qtiles, const int *__restrict__ tot,
                                                           int2 *__restrict__ tmin /* nullable: per (query, tile) bounds for the replay, as scan3_kernel writes them */, int r_lo, int r_hi,
                                                           const uint32_t *__restrict__ cp, int4 *__restrict__ rt,
                                                           uint32_t *__restrict__ ext /* nullable: the other two counters of every pair (scan2_extras) */, uint32_t *__restrict__ rtp /* with ext and CONS: the pre-score packed */, uint4 *__restrict__ tb8 /* with ext: the bounds the replay reads */,
                                                           const int *__restrict__ amb /* side rows, tile 0 of db */,
                                                           const uint32_t *__restrict__ qfull, const int *__restrict__ amb_q, int nq)
{
  // One block = one tile of 64 references; its four waves take a quarter of the word groups each and add their counts up in LDS.
  // (A wave that walks a whole sequence is a chain of a few hundred dependent plane loads: 0.6 ms whatever the launch size -- the
  // floor of every short launch, e.g. the first slice of a search of few queries, which the ordered replay waits for.)
  __shared__ int red[2 * QT + 4][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int qtile, trel;
  if (!scan_work_item(n_qtiles, n_tiles, qtile, trel)) return;
  const int q0 = qtile * QT;
  int acc[QT][2];
#pragma unroll
  for (int q = 0; q < QT; q++) { acc[q][0] = acc[q][1] = 0; }
  const uint4 *t = db + (size_t)(tile_first + trel) * W4 * 4 * 64 + lane;
  const size_t qstride = (size_t)W4 * 16;
  const uint32_t *qb = qp2 + (size_t)q0 * qstride;
  int cc0 = 0, cc1 = 0, cc2 = 0, cc3 = 0;                     // consensus pre-score (CONS, first query tile only)
  // (Requesting the next word group's planes a group ahead, which pays in the rebuild and in the radius search's first stage, changes nothing
  // here even where the registers are free -- one to four queries, 54-61 of 64 registers, eight waves per SIMD either way: 2.66-2.68 against
  // 2.67-2.73 ms per step at one query, 3.00-3.01 against 2.96-3.02 at four, round 4 -- and costs the 16-query kernel two of its seven waves
  // per SIMD: 4.47 against 4.16 ms per step at 16 queries, 7.57 against 7.15 at 32, 3.32 against 3.29 at eight: not done.  The 16-query kernel
  // is bound by its vector instructions: 1.6 G wave-instructions per million references (SQ_INSTS_VALU, profiles/r04_pmc_q16_*) = 2.6 ms of
  // the chip's VALU pipes against 3.8 ms of launches -- 16 per query and word group are the counting itself, 44 decode the planes, about 70
  // the consensus pre-score.  Requesting the words of four queries at once (one wait per four instead of per two) changes nothing either
  // (4.16 ms, and 13 spilled scalar registers).)
  for (int w4 = W4 * wave / 4; w4 < W4 * (wave + 1) / 4; w4++) {
    // (every packed byte is read once per query tile: streaming loads, nothing of it is worth a line of L2)
    const uint4 pA = ld_stream(t + (size_t)(w4 * 4 + 0) * 64), pC = ld_stream(t + (size_t)(w4 * 4 + 1) * 64), pG = ld_stream(t + (size_t)(w4 * 4 + 2) * 64), pT = ld_stream(t + (size_t)(w4 * 4 + 3) * 64);
    const uint32_t rA[4] = {pA.x, pA.y, pA.z, pA.w}, rC[4] = {pC.x, pC.y, pC.z, pC.w}, rG[4] = {pG.x, pG.y, pG.z, pG.w}, rT[4] = {pT.x, pT.y, pT.z, pT.w};
    if (CONS && qtile == 0) {
      const uint32_t *sc = cp + (size_t)w4 * 4 * 6;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t r4[4] = {rA[j], rC[j], rG[j], rT[j]};
        uint32_t k0, k1, k2, k3, M;
        consensus_word<false>(r4, sc + j * 6, k0, k1, k2, k3, M);
        cc0 = bcnt_acc(k0, cc0); cc1 = bcnt_acc(k1, cc1); cc2 = bcnt_acc(k2, cc2); cc3 = bcnt_acc(k3, cc3);
      }
    }
    uint32_t rL[4], rH[4], rI[4], rV[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t par = B3(rA[j], rC[j], rG[j], TT_A ^ TT_B ^ TT_C) ^ rT[j];                 // odd number of set planes
      const uint32_t ac = rA[j] & rC[j], gt = rG[j] & rT[j];
      const uint32_t three = B3(ac, rG[j], rT[j], TT_A & (TT_B | TT_C)) | B3(gt, rA[j], rC[j], TT_A & (TT_B | TT_C));
      rI[j] = par & ~three;                                                                      // exactly one plane set
      rL[j] = B3(rC[j], rT[j], rI[j], (TT_A | TT_B) & TT_C);                                     // A=0 C=1 G=2 T=3
      rH[j] = B3(rG[j], rT[j], rI[j], (TT_A | TT_B) & TT_C);
      rV[j] = B3(rA[j], rC[j], rG[j], TT_A | TT_B | TT_C) | rT[j];
    }
    const uint32_t *s0 = qb + (size_t)w4 * 16;
    QWords<16> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int q = 0; q < QT; q++) {
      if (q + 1 < QT) load_qwords(nxt, s0 + (size_t)(q + 1) * qstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t qL = cur.v[j * 4 + 0], qH = cur.v[j * 4 + 1], qI = cur.v[j * 4 + 2];
        const uint32_t d = rL[j] ^ qL;
        const uint32_t y = B3(rH[j], qH, d, (TT_A ^ TT_B) | TT_C);
        acc[q][0] = bcnt_acc(B3(y, rI[j], qI, ~TT_A & TT_B & TT_C), acc[q][0]);
      }
      // valid pairs = valid(reference) - #(reference valid & query invalid): only word groups where this query has an invalid
      // site can contribute (N runs, gaps, the trimmed ends) -- a wave-uniform test on scalar registers
      if (~(cur.v[3] & cur.v[7] & cur.v[11] & cur.v[15]) != 0u) {
#pragma unroll
        for (int j = 0; j < 4; j++) acc[q][1] = bcnt_acc(rV[j] & ~cur.v[j * 4 + 3], acc[q][1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (q + 1 < QT) cur = nxt;
    }
  }
  scan2_finish<QT, false, CONS>(red, acc, cc0, cc1, cc2, cc3, out, ppad, tot, tmin, r_lo, r_hi, rt, q0, qtile, trel, lane, wave, rtp, ext ? tb8 : nullptr);
  if (ext) scan2_extras<QT>(db, tile_first + trel, trel, W4, amb, qfull, amb_q, q0, nq, ext, ppad, lane, wave);
}

template <int QT, bool CONS>
__global__ __launch_bounds__(256) void scan2_acgt_kernel(const uint4 *__restrict__ db, long long tile_first, int n_tiles, int W4,
                                                          const uint32_t *__restrict__ qp, uint32_t *__restrict__ out, int ppad, int n_qtiles, const int *__restrict__ tot,
                                                          int2 *__restrict__ tmin, int r_lo, int r_hi, const uint32_t *__restrict__ cp, int4 *__restrict__ rt)
{
  __shared__ int red[2 * QT + 4][64];                         // block = one tile of references, the word groups cut among its four waves (see scan2_iupac_kernel)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int qtile, trel;
  if (!scan_work_item(n_qtiles, n_tiles, qtile, trel)) return;
  const int q0 = qtile * QT;
  int acc[QT][2];
#pragma unroll
  for (int q = 0; q < QT; q++) { acc[q][0] = acc[q][1] = 0; }
  const uint4 *t = db + (size_t)(tile_first + trel) * W4 * 3 * 64 + lane;
  const size_t qstride = (size_t)W4 * 16;
  const uint32_t *qb = qp + (size_t)q0 * qstride;
  int cc0 = 0, cc1 = 0;                                       // consensus pre-score (CONS, first query tile only)
  for (int w4 = W4 * wave / 4; w4 < W4 * (wave + 1) / 4; w4++) {
    const uint4 pL = ld_stream(t + (size_t)(w4 * 3 + 0) * 64), pH = ld_stream(t + (size_t)(w4 * 3 + 1) * 64), pI = ld_stream(t + (size_t)(w4 * 3 + 2) * 64);
    const uint32_t rL[4] = {pL.x, pL.y, pL.z, pL.w}, rH[4] = {pH.x, pH.y, pH.z, pH.w}, rI[4] = {pI.x, pI.y, pI.z, pI.w};
    if (CONS && qtile == 0) {
      const uint32_t *sc = cp + (size_t)w4 * 4 * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t r4[4] = {rL[j], rH[j], rI[j], 0u};
        uint32_t k0, k1, k2, k3, M;
        consensus_word<true>(r4, sc + j * 4, k0, k1, k2, k3, M);
        cc0 = bcnt_acc(k0, cc0); cc1 = bcnt_acc(k1, cc1);
      }
    }
    const uint32_t *s0 = qb + (size_t)w4 * 16;
    QWords<16> cur, nxt;
    load_qwords(cur, s0);
#pragma unroll
    for (int q = 0; q < QT; q++) {
      if (q + 1 < QT) load_qwords(nxt, s0 + (size_t)(q + 1) * qstride);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t qL = cur.v[j * 4 + 0], qH = cur.v[j * 4 + 1], qI = cur.v[j * 4 + 2];
        const uint32_t d = rL[j] ^ qL;
        const uint32_t y = B3(rH[j], qH, d, (TT_A ^ TT_B) | TT_C);
        acc[q][0] = bcnt_acc(B3(y, rI[j], qI, TT_A & TT_B & TT_C), acc[q][0]);
      }
      // comparable sites = ACGT(reference) - #(reference ACGT & query not ACGT): only groups where the query is not all ACGT
      if (~(cur.v[2] & cur.v[6] & cur.v[10] & cur.v[14]) != 0u) {
#pragma unroll
        for (int j = 0; j < 4; j++) acc[q][1] = bcnt_acc(rI[j] & ~cur.v[j * 4 + 2], acc[q][1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (q + 1 < QT) cur = nxt;
    }
  }
  scan2_finish<QT, true, CONS>(red, acc, cc0, cc1, 0, 0, out, ppad, tot, tmin, r_lo, r_hi, rt, q0, qtile, trel, lane, wave);
}
