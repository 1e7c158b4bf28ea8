// kernels_scan3.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): derived planes and the column-compressed scan (production path).

// ------------------------------------------------------------------------------------------------------------
// device: column-compressed two-counter scan (production path)
// ------------------------------------------------------------------------------------------------------------
// uvaia compares each reference once against a consensus of the queries on the columns where the queries agree
// (src/nearest.c:428-433, src/fastaseq.c:744-768).  The same idea, restated for bit-planes and kept exact for every pair:
//   * a column is CONSTANT if all queries that are ACGT there carry the same base b (queries that are N/gap/ambiguous there
//     simply do not count), POLYMORPHIC if two queries carry different bases.
//   * constant columns:   ACGT matches(q,r) = popc(E_r & qI) = popc(E_r) - popc(E_r & ~qI),   E_r = [r is ACGT and equals b]
//                         (--acgt: mismatches = popc(D_r & qI), D_r = [r is ACGT and differs from b])
//     so, exactly like the valid-pair count, only the word groups where the query is NOT ACGT cost anything;
//   * polymorphic columns (typically 14-25 % of the alignment) are bit-gathered into contiguous words and compared densely.
// derive_all_kernel builds the per-reference planes for a given query set; scan3_kernel consumes them.

// derive_all_kernel: the E / V planes, the group counts and the gathered polymorphic and rare columns in one pass over the packed planes (each byte of a
// reference read once).
// One block of NWV waves (4, 8 or 16) per tile; wave v takes the contiguous word groups split[v] .. split[v+1]-1 (none where the
// alignment has fewer groups than the block has waves), writes their E/V planes and group counts, and bit-gathers the dense polymorphic
// and the rare columns it meets, one 32-bit word of the gathered planes at a time.  A wave's gathered bits start at a bit position the
// host computed (split[NWV+1+v] dense, split[2(NWV+1)+v] rare); the output words that hold bits of several waves -- a wave's first and
// its last word at most, NWV-1 per section in all -- are OR-ed together in LDS and written after the barrier by the wave behind the
// lowest boundary inside the word, every other word goes straight to memory.  Kept under 64 VGPRs: every tile of a 100 000-reference
// database is resident at once.  The block's width only decides how long a wave's chain of dependent loads is (58 groups at 4 waves and
// 30 000 columns, 15 at 16), which measured makes no difference to a launch's time (DESIGN.md 4.2; four is the default): the arrays it
// writes are the same byte for byte.
//   split[3 (NWV + 1)] = { w4 boundaries [NWV+1], dense bits before each boundary [NWV+1], rare bits before each boundary [NWV+1] }: the
//   section for NWV of the context's table (build_derive_split)
typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ void st_stream(uint4 *p, const uint4 &v)
{ // written once, read by a later kernel: no reason to keep the lines in L2
  const u32x4_nt x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4_nt *>(p));
}
struct GatherStage { uint32_t bL, bH, bI; int fill, ow; };

template <int NWV>
static __device__ __forceinline__ int shared_slot(const int *__restrict__ bit, int word)
{ // boundary 1..NWV-1 that lies inside output word `word` (lowest such: with many waves and few columns several may), or 0
  for (int k = 1; k < NWV; k++) if ((bit[k] & 31) != 0 && (bit[k] >> 5) == word) return k;
  return 0;
}
// one bit of x (uniform position b) moved to bit `at` and merged into acc: v_bfe_u32 + v_lshl_or_b32
static __device__ __forceinline__ uint32_t take_bit(uint32_t x, int b, int at, uint32_t acc)
{
  return (__builtin_amdgcn_ubfe(x, (uint32_t)b, 1u) << at) | acc;
}

// WRITE_V = false: the V plane of every group is in place already (it does not depend on the query set: written when the rows
// were appended) and is left alone; E, the group counts and the gathered planes are rebuilt.
template <bool ACGT, bool WRITE_V, int NWV>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(8, 8)))
void derive_all_kernel(const uint4 *__restrict__ tiles, long long tile_base, long long dtile_base, int W4,
                       const uint32_t *__restrict__ cls, const uint32_t *__restrict__ rmask,
                       const int *__restrict__ split, int NP4, int NR4,
                       uint4 *__restrict__ ev, int *__restrict__ tot_e, uint32_t *__restrict__ grp, uint4 *__restrict__ poly)
{
  constexpr int P = ACGT ? 3 : 4;
  __shared__ int partial[NWV][64];
  __shared__ uint32_t shr[2 * (NWV - 1)][3][64];   // [section * (NWV - 1) + boundary - 1][plane][lane]
  for (int i = threadIdx.x; i < 2 * (NWV - 1) * 3 * 64; i += 64 * NWV) (&shr[0][0][0])[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // packed tile read / tile of the derived arrays written: the same number unless the references are sharded over several GPUs
  // (then a context keeps derived planes only for the tiles it scans, numbered densely: uvaia_gpu_db_set_shard)
  const long long ptile = tile_base + blockIdx.x, tile = dtile_base + blockIdx.x;
  const uint4 *t = tiles + (size_t)ptile * W4 * P * 64 + lane;
  uint4 *o = ev + (size_t)tile * W4 * 2 * 64 + lane;
  const int NG = NP4 + NR4;
  uint32_t *po = reinterpret_cast<uint32_t *>(poly + (size_t)tile * NG * 3 * 64 + lane);   // word j of group g, plane p: po[((g*3+p)*64)*4 + j]
  const int lo = split[wv], hi = split[wv + 1];
  const int *dbit = split + (NWV + 1), *rbit = split + 2 * (NWV + 1);

  GatherStage D, R;
  D.bL = D.bH = D.bI = 0u; D.fill = dbit[wv] & 31; D.ow = dbit[wv] >> 5;
  R.bL = R.bH = R.bI = 0u; R.fill = rbit[wv] & 31; R.ow = rbit[wv] >> 5;
  // The output words this wave shares with others, per section: its first one (the boundary before it falls inside a word) and its last
  // one (the boundary behind it does); -1: none.  sk = the LDS slot of that word: the lowest boundary inside it (a word may hold the bits
  // of more than two waves, and then the first and the last word of a wave in the middle are the same one).
  int sw[2][2], sk[2][2];
#pragma unroll
  for (int sec = 0; sec < 2; sec++) {
    const int *bit = sec ? rbit : dbit;
    sw[sec][0] = (bit[wv] & 31) != 0 ? (bit[wv] >> 5) : -1;
    sw[sec][1] = (wv + 1 < NWV && (bit[wv + 1] & 31) != 0) ? (bit[wv + 1] >> 5) : -1;
#pragma unroll
    for (int e = 0; e < 2; e++) sk[sec][e] = sw[sec][e] >= 0 ? shared_slot<NWV>(bit, sw[sec][e]) : 0;
  }
  auto push_word = [&](GatherStage &g, int sec) {     // the staged bits are word ow of the section's gathered planes
    const int k = (sw[sec][0] == g.ow) ? sk[sec][0] : (sw[sec][1] == g.ow) ? sk[sec][1] : 0;
    if (k) {
      uint32_t (*dst)[64] = shr[sec * (NWV - 1) + k - 1];
      if (g.bL) atomicOr(&dst[0][lane], g.bL);
      if (g.bH) atomicOr(&dst[1][lane], g.bH);
      if (g.bI) atomicOr(&dst[2][lane], g.bI);
    } else {
      uint32_t *d = po + (size_t)((sec ? NP4 : 0) + (g.ow >> 2)) * 3 * 256 + (g.ow & 3);
      d[0] = g.bL; d[256] = g.bH; d[512] = g.bI;
    }
    g.bL = g.bH = g.bI = 0u; g.fill = 0; g.ow++;
  };

  int te = 0;
  // (the packed planes are read once: streaming loads; the next group's planes are requested before this group is worked on -- a rebuild
  // of config[1]'s 100 000 references is three launches of two blocks per CU, too few waves to keep HBM busy with one group each)
  uint4 nxt[P];
#pragma unroll
  for (int p = 0; p < P; p++) nxt[p] = lo < hi ? ld_stream(t + (size_t)(lo * P + p) * 64) : make_uint4(0u, 0u, 0u, 0u);
  for (int w4 = lo; w4 < hi; w4++) {
    uint4 pl[P];
#pragma unroll
    for (int p = 0; p < P; p++) pl[p] = nxt[p];
    if (w4 + 1 < hi) {
#pragma unroll
      for (int p = 0; p < P; p++) nxt[p] = ld_stream(t + (size_t)((w4 + 1) * P + p) * 64);
    }
    uint32_t e[4], v[4];
    int ge = 0, gv = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t rL, rH, rI, rV;
      if (ACGT) { rL = u4c(pl[0], j); rH = u4c(pl[1], j); rI = u4c(pl[2], j); rV = rI; }
      else {
        const uint32_t a = u4c(pl[0], j), cc = u4c(pl[1], j), g = u4c(pl[2], j), tt = u4c(pl[P - 1], j);
        const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
        rI = par & ~three; rL = (cc | tt) & rI; rH = (g | tt) & rI; rV = a | cc | g | tt;
      }
      const uint32_t *c4 = cls + (size_t)(w4 * 4 + j) * 4;
      const uint32_t diff = (rL ^ c4[0]) | (rH ^ c4[1]);
      e[j] = rI & c4[2] & (ACGT ? diff : ~diff);
      v[j] = rV;
      ge += __popc(e[j]); gv += __popc(v[j]);
      for (uint32_t m = c4[3]; m; m &= m - 1) {                         // dense polymorphic columns of the word (uniform loop)
        const int b = __ffs(m) - 1;
        D.bL = take_bit(rL, b, D.fill, D.bL); D.bH = take_bit(rH, b, D.fill, D.bH); D.bI = take_bit(rI, b, D.fill, D.bI);
        if (++D.fill == 32) push_word(D, 0);
      }
      for (uint32_t m = rmask[w4 * 4 + j]; m; m &= m - 1) {             // rare columns
        const int b = __ffs(m) - 1;
        R.bL = take_bit(rL, b, R.fill, R.bL); R.bH = take_bit(rH, b, R.fill, R.bH); R.bI = take_bit(rI, b, R.fill, R.bI);
        if (++R.fill == 32) push_word(R, 1);
      }
    }
    te += ge;
    __builtin_nontemporal_store((uint32_t)ge | ((uint32_t)gv << 16), grp + ((size_t)tile * W4 + w4) * 64 + lane);
    st_stream(o + (size_t)(w4 * 2 + 0) * 64, make_uint4(e[0], e[1], e[2], e[3]));
    if (WRITE_V) st_stream(o + (size_t)(w4 * 2 + 1) * 64, make_uint4(v[0], v[1], v[2], v[3]));
  }
  if (NP4 && D.fill > 0) push_word(D, 0);            // the last, incomplete word of this wave's columns
  if (NR4 && R.fill > 0) push_word(R, 1);
  if (wv == NWV - 1) {                               // zero words that complete the last group of each section
    for (int w = (dbit[NWV] + 31) >> 5; w < NP4 * 4; w++) { uint32_t *d = po + (size_t)(w >> 2) * 3 * 256 + (w & 3); d[0] = 0u; d[256] = 0u; d[512] = 0u; }
    for (int w = (rbit[NWV] + 31) >> 5; w < NR4 * 4; w++) { uint32_t *d = po + (size_t)(NP4 + (w >> 2)) * 3 * 256 + (w & 3); d[0] = 0u; d[256] = 0u; d[512] = 0u; }
  }
  partial[wv][lane] = te;
  __syncthreads();
  if (wv == 0) {
    int t_all = 0;
#pragma unroll
    for (int v = 0; v < NWV; v++) t_all += partial[v][lane];
    tot_e[tile * 64 + lane] = t_all;
  } else {
    // wave k writes the word shared across boundary k (once per word: the lowest boundary inside it owns it) -- also a wave without word
    // groups of its own, which has come here all the same
    for (int sec = 0; sec < 2; sec++) {
      if ((sec ? NR4 : NP4) == 0 || sw[sec][0] < 0 || sk[sec][0] != wv) continue;
      const int w = sw[sec][0];
      const uint32_t (*src)[64] = shr[sec * (NWV - 1) + wv - 1];
      uint32_t *d = po + (size_t)((sec ? NP4 : 0) + (w >> 2)) * 3 * 256 + (w & 3);
      d[0] = src[0][lane]; d[256] = src[1][lane]; d[512] = src[2][lane];
    }
  }
}

// scan over the derived planes.  Two loops per (16 queries x R x 64 references) pass of a wave:
//  1. polymorphic columns, dense: static 16-query unroll, counts in VGPRs, query words by scalar loads (VALU-bound);
//  2. constant columns + validity: only where a query is "dirty".  Measured (profiles/r01_issue_rate_microbench.txt): a CU
//     issues ONE scalar-ALU instruction per cycle for all four SIMDs, and VALU + SALU together ~1.9 per cycle, so a statically
//     unrolled chain of per-query bit tests is bound by its scalar bookkeeping, not by the popcounts.  The dirty work is
//     therefore a precomputed, query-tile-specific ITEM STREAM walked by a dynamic loop: every item carries its eight mask
//     words and the LDS offset of its query's counter, the counters (two u16 halves in one dword: constant-column deficit |
//     validity deficit << 16) live in LDS and take one LDS add per item, and a query that is N/gap over a whole 128-column
//     group costs a single add of the reference's own per-group counts (grp[]).
//  R reference tiles per wave (R = 2 in production): the walk of the stream -- scalar loads, waits, pointer arithmetic, loop
//  branches: two thirds of the instructions issued at R = 1 (profiles/r01_pmc_traffic.json) -- is shared by R x 64 references,
//  and the counters of the R tiles of a (query, lane) sit side by side in LDS so that ONE ds_add_u64 serves both.
//   out = first | second << 16:  first = ACGT matches (default) or ACGT mismatches (--acgt),  second = valid pairs (default) or comparable sites (--acgt)
// One block = one SUPER-TILE of 64 queries x R x 64 references.  The four waves share the counters (one block of LDS: 65 rows of
// R x 64 lanes) and ONE item stream; each wave walks a contiguous share of the stream's records (cut by the host so that the shares
// cost about the same) and adds into the shared counters with LDS atomics.  What a record costs before its first item -- header,
// plane addresses, three plane loads per reference tile, loop set-up: half of all instructions when a wave walked the records of its
// own 16 queries (the ablation in profiles/r02_scan_ablation.json) -- is now paid once per 64 queries, and every plane is loaded
// once per block instead of once per 16 queries.  The polymorphic columns (phase 1) and the epilogue are split by query: wave w
// takes queries 16 w .. 16 w + 15 of the super-tile.
// stream (dwords), per super-tile; sdir[stile][4 NW] = for wave w: {first dword of its group records, their number} at [2w], then
// {first dword of its rare records, their number} at [2 NW + 2w]:
//   record = { w4 * 2048 (byte offset of the group's E plane in the tile, V plane 1 KiB further; the group's grp[] row sits at byte offset
//              w4 * 256) | bit 0: some word item of the record is a run item,
//              n_full4 = ceil(n_full / 4) | n_generic << 16,
//              word-item counts of the group's four words, 8 bits each,
//              length of the record in dwords }
//            + 4 n_full4 LDS offsets of the queries that are all-N in the group (padded with the scratch row)
//            + n_generic x { ~qI & constMask [4],  ~qV (default) / ~qI (--acgt) [4],  LDS offset, 0, 0, 0 }
//            + word items { ~qI & constMask, ~qV, LDS offset, byte mask of the group's full words } of the queries that are dirty in ONE
//              word of the group only, or whose other dirty words hold no valid query character (run items: a non-zero byte mask, those
//              words give the reference's own counts), listed word by word
//   two zero headers { 0, 0, 0, 4 } end the group records of a super-tile (the walk runs two headers ahead)
//   rare record (after them) = { byte offset of a rare group's planes in the tile's gathered planes, word-item counts of 8 bits each, 0, 0 }
//            + items { sites, their lo bits, their hi bits, LDS offset }, word by word
//   LDS offsets are byte offsets of a query's counter row inside the block's counters: (query within the super-tile) * 256 * R
//   (the host builds the stream for the R the context runs); the scratch row is row 64.
//   The whole stream is padded by 64 dwords: items and headers are requested past the end.
// qpl[q][p4][L,H,I,-][4]: compressed planes of the polymorphic columns
template <int R> struct Scan3Acc;
template <> struct Scan3Acc<1> { typedef uint32_t type; };
template <> struct Scan3Acc<2> { typedef unsigned long long type; };
struct Scan3Acc4 { unsigned long long a, b; };                // four tiles: two 64-bit halves, one LDS add each
template <> struct Scan3Acc<4> { typedef Scan3Acc4 type; };
static __device__ __forceinline__ uint32_t acc_part(uint32_t v, int) { return v; }
static __device__ __forceinline__ uint32_t acc_part(unsigned long long v, int rr) { return (uint32_t)(v >> (32 * rr)); }
static __device__ __forceinline__ uint32_t acc_part(const Scan3Acc4 &v, int rr) { return (uint32_t)((rr < 2 ? v.a : v.b) >> (32 * (rr & 1))); }
typedef __attribute__((address_space(3))) char scan3_lds_char;
static __device__ __forceinline__ void lds_counter_add(scan3_lds_char *p, uint32_t v)
{ __hip_atomic_fetch_add((__attribute__((address_space(3))) uint32_t *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
static __device__ __forceinline__ void lds_counter_add(scan3_lds_char *p, unsigned long long v)
{ __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned long long *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
static __device__ __forceinline__ void lds_counter_add(scan3_lds_char *p, const Scan3Acc4 &v)
{
  __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned long long *)p, v.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned long long *)(p + 8), v.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class T> static __device__ __forceinline__ void lds_counter_store(scan3_lds_char *p, const T &v) { *(__attribute__((address_space(3))) T *)p = v; }
static __device__ __forceinline__ void lds_counter_store(scan3_lds_char *p, const Scan3Acc4 &v)
{ *(__attribute__((address_space(3))) unsigned long long *)p = v.a; *(__attribute__((address_space(3))) unsigned long long *)(p + 8) = v.b; }
template <class T> static __device__ __forceinline__ void lds_counter_load(scan3_lds_char *p, T &v) { v = *(__attribute__((address_space(3))) T *)p; }
static __device__ __forceinline__ void lds_counter_load(scan3_lds_char *p, Scan3Acc4 &v)
{ v.a = *(__attribute__((address_space(3))) unsigned long long *)p; v.b = *(__attribute__((address_space(3))) unsigned long long *)(p + 8); }
static __device__ __forceinline__ void lds_counter_sub(scan3_lds_char *p, uint32_t v)
{ __hip_atomic_fetch_sub((__attribute__((address_space(3))) uint32_t *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
static __device__ __forceinline__ void lds_counter_sub(scan3_lds_char *p, unsigned long long v)
{ __hip_atomic_fetch_sub((__attribute__((address_space(3))) unsigned long long *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
static __device__ __forceinline__ void lds_counter_sub(scan3_lds_char *p, const Scan3Acc4 &v)
{
  __hip_atomic_fetch_sub((__attribute__((address_space(3))) unsigned long long *)p, v.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_sub((__attribute__((address_space(3))) unsigned long long *)(p + 8), v.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int NW /* waves per block */, bool ACGT, int R, int QS = 64 /* queries of a super-tile */>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 8))) void scan3_kernel(const uint4 *__restrict__ ev, const uint4 *__restrict__ poly, long long tile_first, int n_tiles,
                                                     int W4, int NP4, int NPT, const uint32_t *__restrict__ qpl, const uint32_t *__restrict__ stream,
                                                     const uint32_t *__restrict__ sdir, const uint32_t *__restrict__ grp,
                                                     const int *__restrict__ tot_e, const int *__restrict__ tot_v,
                                                     uint32_t *__restrict__ out, int ppad, int n_stiles, int2 *__restrict__ tmin, int r_lo, int r_hi,
                                                     int stile_first)
{
  constexpr int QT = QS / NW;                                  // queries a wave takes in phase 1 and in the epilogue
  static_assert((NW == 4 || NW == 8 || NW == 16) && (QS == 64 || QS == 128) && QT >= 4 && QT <= 16, "waves and queries of a super-tile");
  static_assert(R == 1 || R == 2 || R == 4, "one, two or four reference tiles per wave");
  typedef typename Scan3Acc<R>::type acc_t;
  constexpr uint32_t RARE_BIAS = SCAN3_BIAS;                 // the low counter half also takes what the rare items (and, --acgt, the polymorphic columns) give back: keep it positive
  __shared__ acc_t lacc[QS + 1][64];                           // the block's counters: one packed counter per (query, lane, tile of the block) + a scratch row
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform by construction: say so
  int stile, group;
  if (!scan_work_item(n_stiles, (n_tiles + R - 1) / R, stile, group)) return;
  const int trel0 = group * R;
  stile += stile_first;                                        // only the active super-tiles are scanned (query shards)
  const int q0 = stile * QS + wave * QT;                       // this wave's queries in phase 1 and in the epilogue
  // tile rr of this wave; a wave whose second tile lies past the end recounts its first one (nothing of it is stored)
  int trel[R]; bool live[R];
#pragma unroll
  for (int rr = 0; rr < R; rr++) { live[rr] = trel0 + rr < n_tiles; trel[rr] = live[rr] ? trel0 + rr : trel0; }
  // explicit LDS pointers: the stream loads stay scalar (no may-alias with the atomics)
  scan3_lds_char *my = (scan3_lds_char *)&lacc[wave * QT][lane];             // rows of this wave's queries (a row = 64 * sizeof(acc_t) bytes)
  auto pack_acc = [](const uint32_t (&v)[R]) -> acc_t {
    if constexpr (R == 1) return v[0];
    else if constexpr (R == 2) return (acc_t)v[0] | ((acc_t)v[1] << 32);
    else return acc_t{(unsigned long long)v[0] | ((unsigned long long)v[1] << 32), (unsigned long long)v[2] | ((unsigned long long)v[3] << 32)};
  };
  {
    int acc[R][QT];
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
      for (int q = 0; q < QT; q++) acc[rr][q] = 0;
    // ---- polymorphic columns, dense
    {
      const uint4 *t[R];
#pragma unroll
      for (int rr = 0; rr < R; rr++) t[rr] = poly + (size_t)(tile_first + trel[rr]) * NPT * 3 * 64 + lane;
      const size_t qstride = (size_t)NP4 * 16;
      const uint32_t *qb = qpl + (size_t)q0 * qstride;
      for (int p4 = 0; p4 < NP4; p4++) {
        uint4 pL[R], pH[R], pI[R];
#pragma unroll
        for (int rr = 0; rr < R; rr++) { pL[rr] = t[rr][(size_t)(p4 * 3 + 0) * 64]; pH[rr] = t[rr][(size_t)(p4 * 3 + 1) * 64]; pI[rr] = t[rr][(size_t)(p4 * 3 + 2) * 64]; }
        const uint32_t *s0 = qb + (size_t)p4 * 16;
        QWords<12> cur, nxt;                                  // L[4], H[4], I[4] of the group: one s_load_dwordx8 + one x4
        load_qwords(cur, s0);
#pragma unroll
        for (int q = 0; q < QT; q++) {
          if (q + 1 < QT) load_qwords(nxt, s0 + (size_t)(q + 1) * qstride);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int rr = 0; rr < R; rr++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const uint32_t d = u4c(pL[rr], j) ^ cur.v[j];
              const uint32_t y = B3(u4c(pH[rr], j), cur.v[4 + j], d, (TT_A ^ TT_B) | TT_C);
              // --acgt: mismatches (they are also dist_unique).  default: NON-matches (padding bits included), which start the
              // constant-column deficit:  matches = te + 128 NP4 - (non-matches here + what the dirty words take away)
              acc[rr][q] = bcnt_acc(ACGT ? B3(y, u4c(pI[rr], j), cur.v[8 + j], TT_A & TT_B & TT_C) : B3(y, u4c(pI[rr], j), cur.v[8 + j], ~(~TT_A & TT_B & TT_C)), acc[rr][q]);
            }
          __builtin_amdgcn_sched_barrier(0);
          if (q + 1 < QT) cur = nxt;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < QT; q++) {
      uint32_t init[R];
#pragma unroll
      for (int rr = 0; rr < R; rr++) {
        // --acgt: the mismatches on the polymorphic columns are part of the pair's mismatch count: a negative deficit (the replay counts
        // them again for the pairs that reach a heap, where they are dist_unique: src/nearest.c:469)
        if (ACGT) init[rr] = RARE_BIAS - (uint32_t)acc[rr][q];
        else init[rr] = (uint32_t)acc[rr][q] + RARE_BIAS;
      }
      lds_counter_store(my + (size_t)q * 64 * sizeof(acc_t), pack_acc(init));
    }
  }
  __syncthreads();                                             // every counter of the block starts from its polymorphic-column count
  // ---- constant columns and validity: this wave's share of the super-tile's item stream
  {
    const uint4 *t[R]; const uint32_t *gt[R];
#pragma unroll
    for (int rr = 0; rr < R; rr++) { t[rr] = ev + (size_t)(tile_first + trel[rr]) * W4 * 2 * 64 + lane; gt[rr] = grp + (size_t)(tile_first + trel[rr]) * W4 * 64 + lane; }
    typedef __attribute__((address_space(4))) const uint32_t cst_u32;   // constant address space: uniform loads from it are scalar loads
    const cst_u32 *dir = (const cst_u32 *)(sdir + (size_t)stile * 4 * NW);
    const cst_u32 *sp = (const cst_u32 *)(stream + dir[2 * wave]);
    scan3_lds_char *myc = (scan3_lds_char *)&lacc[0][lane];     // the block's counters: the stream's LDS offsets count from row 0
#define LDS_ADD(byte_off, val) lds_counter_add(myc + (byte_off), (val))
#define LDS_SUB(byte_off, val) lds_counter_sub(myc + (byte_off), (val))
#define TOUCH_ITEM(it) asm volatile("" ::"s"(it.v[0]), "s"(it.v[1]), "s"(it.v[2]), "s"(it.v[3]), "s"(it.v[4]), "s"(it.v[5]), "s"(it.v[6]), "s"(it.v[7]), "s"(it.v[8]))
#define TOUCH4(it) asm volatile("" ::"s"(it.v[0]), "s"(it.v[1]), "s"(it.v[2]), "s"(it.v[3]))
    // The planes of a record are requested one record AHEAD (two register sets, the loop is unrolled by two so that the sets swap
    // roles without copies): with two reference tiles per wave only four waves fit a SIMD (the counters in LDS), too few to hide a
    // plane load per record behind other waves.  For that the headers run two records ahead: h = this record, hn = the next one
    // (its planes are requested now), hnn = the one after (requested now, there when the next record starts).  All three planes of
    // a record are loaded whether or not an item needs them (E, V, group counts: a fixed number of loads per record, so that the
    // wait for this record's planes can leave the next record's in flight).
    struct Planes { uint4 E[R], V[R]; uint32_t g[R]; };
    Planes PA, PB;
    auto request = [&](Planes &P, uint32_t h0) {
#pragma unroll
      for (int rr = 0; rr < R; rr++) {
        const char *tg = reinterpret_cast<const char *>(t[rr]) + (h0 & ~1023u);        // E plane of the group, V plane 1 KiB further
        P.E[rr] = *reinterpret_cast<const uint4 *>(tg);
        P.V[rr] = *reinterpret_cast<const uint4 *>(tg + 1024);
        P.g[rr] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(gt[rr]) + ((h0 & ~1023u) >> 3));
      }
    };
    QWords<4> h, hn, hnn;
    load_qwords(h, sp);
    const cst_u32 *sp_n = sp + h.v[3];            // h.v[3]: length of the record in dwords (past the last record: the next tile's first header, or the padding)
    load_qwords(hn, sp_n);
    request(PA, h.v[0]);
    const uint32_t n_rec = dir[2 * wave + 1];
    // one record: items of `h` on the planes in P; the planes of the next record go to Pn
#define RECORD(P, Pn)                                                                                                             \
    {                                                                                                                             \
      const uint32_t n_full4 = h.v[1] & 0xFFFFu, n_gen = h.v[1] >> 16, n_words = h.v[2];                                          \
      const cst_u32 *sp_nn = sp_n + hn.v[3];                                                                                      \
      load_qwords(hnn, sp_nn);                                                                                                    \
      request(Pn, hn.v[0]);                                                                                                       \
      sp += 4;                                                                                                                    \
      /* the first general item and the first word item of the record are requested here as well */                             \
      const cst_u32 *ip = sp + n_full4 * 4u, *wp = ip + n_gen * 12u;                                                              \
      QWords<9> a, b;                                                                                                             \
      QWords<4> it, nx;                                                                                                           \
      load_qwords(a, ip);                                                                                                         \
      load_qwords(it, wp);                                                                                                        \
      if (n_full4) {    /* all-N queries: what they take away is the reference's own count for the group (same packing as the counters) */ \
        const acc_t gg = pack_acc(P.g);                                                                                           \
        _Pragma("unroll 1") for (uint32_t k = 0; k < n_full4; k++, sp += 4) {      /* four LDS offsets per step; the list is padded with a scratch row */ \
          QWords<4> o;                                                                                                            \
          load_qwords(o, sp);                                                                                                     \
          LDS_ADD(o.v[0], gg); LDS_ADD(o.v[1], gg); LDS_ADD(o.v[2], gg); LDS_ADD(o.v[3], gg);                                     \
        }                                                                                                                         \
      }                                                                                                                           \
      if (n_gen) {                                                                                                                \
        /* Two items in flight: the words of the next one arrive while the current one is counted.  The wait for the prefetched item */ \
        /* (TOUCH_ITEM; scalar loads return out of order, so the only wait is "everything", LDS adds included) sits BEFORE the add */ \
        /* of the current item: the add then has a whole item's counting to complete before the next wait looks at it. */         \
        TOUCH_ITEM(a);                                                                                                            \
        for (uint32_t k = 0; k < n_gen; k += 2, ip += 24) {                                                                       \
          acc_t va, vb;                                                                                                           \
          load_qwords(b, ip + 12);       /* the stream is padded: reading past the last item is harmless */                       \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          ITEM_VALUE(P, a, va);                                                                                                   \
          const uint32_t off_a = a.v[8];                                                                                          \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          TOUCH_ITEM(b);                                                                                                          \
          LDS_ADD(off_a, va);                                                                                                     \
          if (k + 1 < n_gen) {                                                                                                    \
            load_qwords(a, ip + 24);                                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                                    \
            ITEM_VALUE(P, b, vb);                                                                                                 \
            const uint32_t off_b = b.v[8];                                                                                        \
            __builtin_amdgcn_sched_barrier(0);                                                                                    \
            TOUCH_ITEM(a);                                                                                                        \
            LDS_ADD(off_b, vb);                                                                                                   \
          }                                                                                                                       \
        }                                                                                                                         \
      }                                                                                                                           \
      if (n_words) {    /* word items, listed word by word: { ~qI & constMask, ~qV, LDS offset, byte mask of the group's full words } */ \
        /* one item ahead across the four lists (they are contiguous in the stream) */                                           \
        uint32_t wE[R], wV[R];      /* per word of the group the popcounts of E and V, one byte each: what a run item adds for its full words */ \
        _Pragma("unroll") for (int rr = 0; rr < R; rr++) { wE[rr] = 0u; wV[rr] = 0u; }                                            \
        if (h.v[0] & 1u) {                                                                                                        \
          _Pragma("unroll") for (int rr = 0; rr < R; rr++) {                                                                      \
            wE[rr] = (uint32_t)bcnt_acc(P.E[rr].x, 0) | (uint32_t)bcnt_acc(P.E[rr].y, 0) << 8 | (uint32_t)bcnt_acc(P.E[rr].z, 0) << 16 | (uint32_t)bcnt_acc(P.E[rr].w, 0) << 24; \
            wV[rr] = (uint32_t)bcnt_acc(P.V[rr].x, 0) | (uint32_t)bcnt_acc(P.V[rr].y, 0) << 8 | (uint32_t)bcnt_acc(P.V[rr].z, 0) << 16 | (uint32_t)bcnt_acc(P.V[rr].w, 0) << 24; \
          }                                                                                                                       \
        }                                                                                                                         \
        TOUCH4(it);                                                                                                               \
        WORD_ITEMS(P, 0) WORD_ITEMS(P, 1) WORD_ITEMS(P, 2) WORD_ITEMS(P, 3)                                                       \
      }                                                                                                                           \
      sp = sp_n; sp_n = sp_nn; h = hn; hn = hnn;                                                                                  \
    }
    // packed deficits of one general item for the R tiles: 8 x (v_and + v_bcnt) + pack per tile
#define ITEM_VALUE(P, it, dst)                                                                                      \
    {                                                                                                               \
      uint32_t pk_[R];                                                                                              \
      _Pragma("unroll") for (int rr = 0; rr < R; rr++) {                                                            \
        int e_ = 0, v_ = 0;                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; j++) e_ = bcnt_acc(u4c(P.E[rr], j) & it.v[j], e_);                 \
        _Pragma("unroll") for (int j = 0; j < 4; j++) v_ = bcnt_acc(u4c(P.V[rr], j) & it.v[4 + j], v_);             \
        pk_[rr] = (uint32_t)e_ | ((uint32_t)v_ << 16);                                                              \
      }                                                                                                             \
      dst = pack_acc(pk_);                                                                                          \
    }
    /* one word item `cur` (the next one, `ahead`, was requested just before: the wait for it sits in front of the LDS add) */     \
#define WORD_ITEM(P, J, cur, ahead)                                                                                               \
        {                                                                                                                         \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          uint32_t pk_[R];                                                                                                        \
          _Pragma("unroll") for (int rr = 0; rr < R; rr++)                                                                        \
            pk_[rr] = (uint32_t)bcnt_acc(u4c(P.E[rr], J) & cur.v[0], 0) | ((uint32_t)bcnt_acc(u4c(P.V[rr], J) & cur.v[1], 0) << 16); \
          if (cur.v[3]) {     /* run item: the group's other dirty words hold no valid query character: the reference's own counts there */ \
            _Pragma("unroll") for (int rr = 0; rr < R; rr++)                                                                      \
              pk_[rr] += __builtin_amdgcn_sad_u8(wE[rr] & cur.v[3], 0u, 0u) | (__builtin_amdgcn_sad_u8(wV[rr] & cur.v[3], 0u, 0u) << 16); \
          }                                                                                                                       \
          const uint32_t off_ = cur.v[2];                                                                                         \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          TOUCH4(ahead);                                                                                                          \
          LDS_ADD(off_, pack_acc(pk_));                                                                                           \
        }
    /* the items of one word, two per trip: `it` and `nx` swap roles inside the trip, so no register copies and half the loop control per */ \
    /* item (the items of the four words are contiguous in the stream: the item after a list's last one is the next list's first)     */ \
#define WORD_ITEMS(P, J)                                                                                                          \
        {                                                                                                                         \
          uint32_t k = (n_words >> (8 * J)) & 255u;                                                                               \
          _Pragma("unroll 1") for (; k >= 2; k -= 2) {                                                                            \
            load_qwords(nx, wp + 4);                                                                                              \
            WORD_ITEM(P, J, it, nx)                                                                                               \
            wp += 8;                                                                                                              \
            load_qwords(it, wp);                                                                                                  \
            WORD_ITEM(P, J, nx, it)                                                                                               \
          }                                                                                                                       \
          if (k) {                                                                                                                \
            wp += 4;                                                                                                              \
            load_qwords(nx, wp);                                                                                                  \
            WORD_ITEM(P, J, it, nx)                                                                                               \
            it = nx;                                                                                                              \
          }                                                                                                                       \
        }
    for (uint32_t rec = 0; rec < n_rec; rec += 2) {
      RECORD(PA, PB)
      if (rec + 1 < n_rec) RECORD(PB, PA)
    }
#undef RECORD
#undef ITEM_VALUE
#undef WORD_ITEMS
#undef WORD_ITEM
    // ---- rare columns: the queries that do not carry a rare column's majority base were made dirty there above (their E bit is
    // taken away); here they get the true comparison on the gathered planes of the rare columns, as a negative deficit.  The
    // the rare records of the super-tile are shared out among the waves like the group records.
    {
      const char *tr[R];
#pragma unroll
      for (int rr = 0; rr < R; rr++) tr[rr] = reinterpret_cast<const char *>(poly + (size_t)(tile_first + trel[rr]) * NPT * 3 * 64 + lane);
      sp = (const cst_u32 *)(stream + dir[2 * NW + 2 * wave]);
      for (uint32_t rec = 0; rec < dir[2 * NW + 2 * wave + 1]; rec++) {
        QWords<2> hr;
        load_qwords(hr, sp);
        sp += 4;
        uint4 pL[R], pH[R], pI[R];
#pragma unroll
        for (int rr = 0; rr < R; rr++) {
          pL[rr] = *reinterpret_cast<const uint4 *>(tr[rr] + hr.v[0]); pH[rr] = *reinterpret_cast<const uint4 *>(tr[rr] + hr.v[0] + 1024);
          pI[rr] = *reinterpret_cast<const uint4 *>(tr[rr] + hr.v[0] + 2048);
        }
        const uint32_t n_words = hr.v[1];
        QWords<4> it, nx;                                       /* sites, their lo bits, their hi bits, LDS offset */
        load_qwords(it, sp);
        TOUCH4(it);
#define RARE_ITEM(J, cur, ahead)                                                                                                  \
        {                                                                                                                         \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          uint32_t c_[R];                                                                                                         \
          _Pragma("unroll") for (int rr = 0; rr < R; rr++) {                                                                      \
            const uint32_t d_ = u4c(pL[rr], J) ^ cur.v[1];                                                                        \
            const uint32_t y_ = B3(u4c(pH[rr], J), cur.v[2], d_, (TT_A ^ TT_B) | TT_C);                                           \
            const uint32_t g_ = ACGT ? B3(y_, u4c(pI[rr], J), cur.v[0], TT_A & TT_B & TT_C) : B3(y_, u4c(pI[rr], J), cur.v[0], ~TT_A & TT_B & TT_C); \
            c_[rr] = (uint32_t)bcnt_acc(g_, 0);                                                                                   \
          }                                                                                                                       \
          const uint32_t off_ = cur.v[3];                                                                                         \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
          TOUCH4(ahead);                                                                                                          \
          LDS_SUB(off_, pack_acc(c_));                            /* matches (default) / mismatches (--acgt) found: deficit goes down */ \
        }
#define RARE_ITEMS(J)                                                                                                             \
        {                                                                                                                         \
          uint32_t k = (n_words >> (8 * J)) & 255u;                                                                               \
          _Pragma("unroll 1") for (; k >= 2; k -= 2) {                                                                            \
            load_qwords(nx, sp + 4);                                                                                              \
            RARE_ITEM(J, it, nx)                                                                                                  \
            sp += 8;                                                                                                              \
            load_qwords(it, sp);                                                                                                  \
            RARE_ITEM(J, nx, it)                                                                                                  \
          }                                                                                                                       \
          if (k) {                                                                                                                \
            sp += 4;                                                                                                              \
            load_qwords(nx, sp);                                                                                                  \
            RARE_ITEM(J, it, nx)                                                                                                  \
            it = nx;                                                                                                              \
          }                                                                                                                       \
        }
        RARE_ITEMS(0) RARE_ITEMS(1) RARE_ITEMS(2) RARE_ITEMS(3)
#undef RARE_ITEMS
#undef RARE_ITEM
      }
    }
#undef LDS_ADD
#undef LDS_SUB
#undef TOUCH_ITEM
#undef TOUCH4
  }
  __syncthreads();                                             // all four waves' items are in the counters
  int te[R], tv[R]; bool in_batch[R]; size_t r[R];
#pragma unroll
  for (int rr = 0; rr < R; rr++) {
    r[rr] = (size_t)trel[rr] * 64 + lane;
    te[rr] = tot_e[r[rr]]; tv[rr] = tot_v[r[rr]];
    in_batch[rr] = ((int)r[rr] >= r_lo && (int)r[rr] < r_hi);
  }
  // What leaves the kernel: one dword per pair (first counter | second << 16) and, per (query, tile of 64 references), two bounds that
  // let the replay skip tiles that cannot admit anything: the smallest mismatch count (the gate of src/nearest.c:488 needs mismatches <
  // tolerance) and the largest ACGT-match count (a full heap only takes a key that is not below its worst one, and ACGT matches are the
  // first key: src/min_heap.c:95).  (Skipping the counters of such tiles HERE was tried in round 3: the scan runs slices ahead of the
  // replay and may only use bounds that never loosen -- largest mismatch count held + 1, first key of the worst kept entry -- and under
  // those 99-100 % of the tiles still qualify; the replay's own test uses the live tolerance, which is not monotone.  DESIGN.md 4.1.)
#pragma unroll
  for (int q = 0; q < QT; q++) {
    acc_t pkk;
    lds_counter_load(my + (size_t)q * 64 * sizeof(acc_t), pkk);
#pragma unroll
    for (int rr = 0; rr < R; rr++) {
      if (!live[rr]) continue;                                          // wave-uniform
      const uint32_t pk = acc_part(pkk, rr);
      const int c0 = (ACGT ? te[rr] : te[rr] + NP4 * 128) - ((int)(pk & 0xFFFFu) - (int)RARE_BIAS), c1 = tv[rr] - (int)(pk >> 16);
      out[(size_t)(q0 + q) * ppad + r[rr]] = (uint32_t)c0 | ((uint32_t)c1 << 16);
      const int mm = ACGT ? c0 : c1 - c0, kk = ACGT ? c1 - c0 : c0;
      // both bounds by DPP (wave_max_dpp: no trip through the LDS crossbar per step); the counts are below 2^16: the smallest mismatch count is
      // the largest of 65 536 - count, 0 standing for "no reference of the batch in this tile"
      const uint32_t mx_m = wave_max_dpp(in_batch[rr] ? 65536u - (uint32_t)mm : 0u), mx_k = wave_max_dpp(in_batch[rr] ? (uint32_t)kk + 1u : 0u);
      const int m = mx_m ? (int)(65536u - mx_m) : 0x7fffffff, k = mx_k ? (int)(mx_k - 1u) : (int)0x80000000;
      if (lane == 0) {
        int2 *tp = tmin + (size_t)(q0 + q) * (ppad >> 6) + trel[rr];
        *tp = make_int2(m, k);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                                // one query at a time: keeps the epilogue from inflating the register budget
  }
}
