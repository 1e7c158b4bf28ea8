// host_launch.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): kernel launch glue -- scans, replays, derived planes, staging and packing of rows -- shared by the entry points.

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
namespace {

// host-side preparation of a query set is O(queries x columns) several times over: spread the independent pieces over threads
template <class F>
static void parallel_for(int n, F f)
{
  const unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 64u);   // (16 until round 2: 0.33 s of a 10 000-query open were these loops)
  if (n < 32 || nt < 2) { for (int i = 0; i < n; i++) f(i); return; }
  std::atomic<int> next(0);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++) th.emplace_back([&]() { for (;;) { const int a = next.fetch_add(4); if (a >= n) break; for (int i = a; i < std::min(n, a + 4); i++) f(i); } });
  for (auto &x : th) x.join();
}

// Query planes restricted to the polymorphic columns (query->idx): what the radius search and the redundancy test compare references
// with.  Packing a query row with every other site left out gives its full planes under the mask of those columns, so they are made
// on the device from d_qp by the first call that needs them.
__global__ void mask_query_planes_kernel(const uint32_t *__restrict__ qp, const uint32_t *__restrict__ pmask, uint32_t *__restrict__ out, size_t n_words_total, int words_per_row, int nq_planes)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_words_total) return;
  const int w = (int)((i / (size_t)nq_planes) % (size_t)words_per_row);       // layout [query][word][plane]
  out[i] = qp[i] & pmask[w];
}

int ensure_qpoly(uvaia_gpu_ctx *c)
{
  if (c->tab.d_qpoly) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->nq_pad * c->W4 * 4 * c->NQ;
  DevBuf<uint32_t> d;
  if (int rc = d.reserve(c, n)) return rc;
  hipLaunchKernelGGL(mask_query_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->st.stream, c->tab.d_qp, c->tab.d_pmask, d, n, c->W4 * 4, c->NQ);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
  if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "query planes on the polymorphic columns: %s", hipGetErrorString(e));
  c->tab.d_qpoly = std::move(d);
  return 0;
}

// The queries on the columns of query->idx, bit-gathered (kernels_ball.inc): what stage 2 of the radius search compares references with.
int ensure_qgather(uvaia_gpu_ctx *c)
{
  if (c->ball.d_qg) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const int NG = c->acgt ? 3 : 5, W = c->W4 * 4, n_idx = c->ball.n_idx;
  // Column order of the gathered words.  The scan drops a query once every reference of the tile has reached its limit against it
  // (ball_scan_kernel), so the columns where sequences differ most often go first: the BALL_HOT_COLS columns with the most queries
  // off the column's most frequent character fill the first word groups, the others follow, each set in increasing column order
  // (the benchmark's queries: a query stays for 1.6 word groups on average instead of 7 of 33).  Distances are sums over columns: the
  // order changes no result.
  constexpr int BALL_HOT_COLS = 256;
  std::vector<int> cols(c->ball.idx_cols.begin(), c->ball.idx_cols.begin() + n_idx), order;
  std::vector<uint32_t> masks((size_t)2 * W, 0u);
  int n_hot = 0;
  if (n_idx >= 2 * BALL_HOT_COLS) {
    DevBuf<int> d_score;
    std::vector<int> score((size_t)n_idx);
    if (int rc = d_score.reserve(c, (size_t)n_idx)) return rc;
    if (c->acgt) hipLaunchKernelGGL((ball_column_diversity_kernel<true>), dim3((n_idx + 63) / 64), dim3(64), 0, c->st.stream, c->tab.d_qp, c->nq, c->W4, c->ball.d_idx_cols, n_idx, d_score);
    else         hipLaunchKernelGGL((ball_column_diversity_kernel<false>), dim3((n_idx + 63) / 64), dim3(64), 0, c->st.stream, c->tab.d_qp, c->nq, c->W4, c->ball.d_idx_cols, n_idx, d_score);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(score.data(), d_score, (size_t)n_idx * sizeof(int), hipMemcpyDeviceToHost, c->st.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
    if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "diversity of the polymorphic columns: %s", hipGetErrorString(e));
    std::vector<int> by_score((size_t)n_idx);
    for (int i = 0; i < n_idx; i++) by_score[(size_t)i] = i;
    std::stable_sort(by_score.begin(), by_score.end(), [&](int a, int b) { return score[(size_t)a] > score[(size_t)b]; });   // ties: the lower column first
    n_hot = BALL_HOT_COLS;
    std::vector<uint8_t> is_hot((size_t)n_idx, 0);
    for (int i = 0; i < n_hot; i++) is_hot[(size_t)by_score[(size_t)i]] = 1;
    for (int i = 0; i < n_idx; i++) if (is_hot[(size_t)i]) order.push_back(cols[(size_t)i]);
    for (int i = 0; i < n_idx; i++) if (!is_hot[(size_t)i]) order.push_back(cols[(size_t)i]);
  } else order = cols;
  c->ball.NH4 = n_hot / 128;
  c->ball.NG4 = std::max(1, c->ball.NH4 + (n_idx - n_hot + 127) / 128);
  for (int i = 0; i < n_idx; i++) { const int col = order[(size_t)i]; masks[(size_t)(col >> 7) * 8 + (i < n_hot ? 0 : 4) + ((col >> 5) & 3)] |= 1u << (col & 31); }   // [word group][hot 4 | others 4]
  // (n_hot is a multiple of 128: the other columns start at a word group of their own)
  order.resize(order.size() + 1, 0);
  DevBuf<uint32_t> d, dm; DevBuf<int> dc;
  const size_t n = (size_t)c->nq_pad * c->ball.NG4 * 4 * NG;
  if (int rc = d.reserve(c, n)) return rc;
  if (int rc = dm.reserve(c, masks.size())) return rc;
  if (int rc = dc.reserve(c, order.size())) return rc;
  hipError_t e = hipMemcpyAsync(dm, masks.data(), masks.size() * 4, hipMemcpyHostToDevice, c->st.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dc, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->st.stream);
  if (e == hipSuccess) e = hipMemsetAsync(d, 0, n * 4, c->st.stream);
  dim3 grid((unsigned)((c->ball.NG4 * 4 + 63) / 64), (unsigned)c->nq);
  if (e == hipSuccess) {
    if (c->acgt) hipLaunchKernelGGL((ball_gather_queries_kernel<true>), grid, dim3(64), 0, c->st.stream, c->tab.d_qp, c->nq, c->W4, dc, n_idx, c->ball.NG4, d);
    else         hipLaunchKernelGGL((ball_gather_queries_kernel<false>), grid, dim3(64), 0, c->st.stream, c->tab.d_qp, c->nq, c->W4, dc, n_idx, c->ball.NG4, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
  if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "query planes on the polymorphic columns: %s", hipGetErrorString(e));
  c->ball.d_qg = std::move(d); c->ball.d_masks = std::move(dm);
  return 0;
}

// a store of `tiles` tiles of 64 references (whatever it held before goes): packed planes, counts and side rows zeroed, the derived planes as they come
int store_alloc(uvaia_gpu_ctx *c, TileStore &s, size_t tiles)
{
  s = TileStore();
  DevBuf<uint4> planes;
  const size_t refs = tiles * 64, tile_u4 = (size_t)c->W4 * c->P * 64;
  if (int rc = s.nonn.reserve(c, refs)) return rc;
  HIPCHK(c, hipMemset(s.nonn, 0, refs * sizeof(int)));
  if (int rc = s.ev.reserve(c, tiles * (size_t)c->W4 * 2 * 64)) return rc;
  if (int rc = s.grp.reserve(c, tiles * (size_t)c->W4 * 64)) return rc;
  if (int rc = s.poly.reserve(c, tiles * (size_t)std::max(c->tab.NP4 + c->tab.NR4, 1) * 3 * 64)) return rc;
  if (int rc = s.tote.reserve(c, refs)) return rc;
  if (int rc = s.tot.reserve(c, refs)) return rc;
  HIPCHK(c, hipMemset(s.tot, 0, refs * sizeof(int)));
  if (int rc = s.amb.reserve(c, refs * AMB_ROW)) return rc;
  HIPCHK(c, hipMemset(s.amb, 0, refs * AMB_ROW * sizeof(int)));
  if (int rc = planes.reserve(c, tiles * tile_u4)) return rc;
  HIPCHK(c, hipMemset(planes, 0, tiles * tile_u4 * sizeof(uint4)));
  // hipMemset of device memory returns before it has run, on the null stream, which the context's own (non-blocking) streams do not wait
  // for: without this wait a pack kernel queued right behind the allocation can be overtaken by the zeroing of the planes it wrote
  HIPCHK(c, hipStreamSynchronize(nullptr));
  s.planes = std::move(planes);                           // last: its presence says all of them are there
  return 0;
}

// Buffers of a streamed batch (uvaia_gpu_push, uvaia_gpu_ball, uvaia_gpu_agree_on_polymorphic): packed tiles of max_pool references,
// the planes derived from them, side rows.  A context that only searches a resident database never needs them.
int ensure_batch_buffers(uvaia_gpu_ctx *c)
{
  if (c->batch.planes) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  return store_alloc(c, c->batch, c->pool_pad / 64);
}

// Packs one character row restricted to `keep` (nullable: keep everything inside [lo,hi)) into query-plane words:
// dst[(w4*4 + j)*NQ + plane].  is_poly marks query->idx columns (--acgt: fourth plane).
int pack_query_row(const uint8_t *code_tab, const char *row, int nchar, int lo, int hi, const uint8_t *keep, const uint8_t *is_poly,
                   bool acgt, int NQ, uint32_t *dst, int *bad_byte)
{
  for (int s = lo; s < hi; s++) {
    if (keep && !keep[s]) continue;
    const uint8_t code = code_tab[(unsigned char)row[s]];
    if (code == 0xFF) { *bad_byte = (unsigned char)row[s]; return -1; }
    if (!code) continue;
    const int w = s >> 5, b = s & 31;
    uint32_t *d = dst + (size_t)w * NQ;      // (w4*4+j) == w
    const bool one = (code & (code - 1)) == 0;
    if (acgt) {
      if (!one) continue;
      const uint32_t two = code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 0u;
      d[0] |= (two & 1u) << b; d[1] |= (two >> 1) << b; d[2] |= 1u << b;
      if (is_poly && is_poly[s]) d[3] |= 1u << b;
    } else {
      for (int p = 0; p < 4; p++) d[p] |= (uint32_t)((code >> p) & 1u) << b;
      d[4] |= 1u << b;
      if (one) d[5] |= 1u << b;
    }
  }
  return 0;
}

// derive_all_kernel's column split (query table 9): for each block width -- 4, 8, 16 waves per tile, in this order -- a section of
// 3 (NWV + 1) ints: the word groups where each wave starts (equal shares of W4, uneven where it is no multiple; a wave has none where
// W4 < NWV), and the dense and the rare gathered bits before each of those boundaries.  One routine for both builders of the tables.
constexpr int DERIVE_SPLIT_INTS = 3 * (5 + 9 + 17);
inline int derive_split_offset(int nwv) { return nwv == 4 ? 0 : nwv == 8 ? 3 * 5 : 3 * (5 + 9); }
inline void build_derive_split(const uint32_t *cls, const uint32_t *rmask, int W4, int *split)
{
  for (int nwv : {4, 8, 16}) {
    int *s = split + derive_split_offset(nwv);
    for (int v = 0; v <= nwv; v++) s[v] = (int)((long long)W4 * v / nwv);
    int nd = 0, nr = 0, w = 0;
    for (int v = 0; v <= nwv; v++) {
      for (; w < s[v] * 4; w++) { nd += __builtin_popcount(cls[(size_t)w * 4 + 3]); nr += __builtin_popcount(rmask[(size_t)w]); }
      s[nwv + 1 + v] = nd; s[2 * (nwv + 1) + v] = nr;
    }
  }
}

// Book-keeping of what uvaia_gpu_db_rederive has to queue behind (uvaia_gpu_ctx::planes_busy): planes_touch = work that reads or writes the
// derived planes goes onto `st` now; planes_fenced = `ev` has just been recorded on `st` (an event re-recorded on another stream no longer
// stands for the stream it was recorded on before); planes_idle = the host has waited for `stream` (main) or for the scan streams.
inline int planes_slot(const uvaia_gpu_ctx *c, hipStream_t st) { for (int i = 0; i < 3; i++) if (st && st == c->st.scan_streams[i]) return 1 + i; return 0; }
inline void planes_touch(uvaia_gpu_ctx *c, hipStream_t st) { const int i = planes_slot(c, st); c->st.planes_busy[i] = true; c->st.planes_ev[i] = nullptr; }
inline void planes_fenced(uvaia_gpu_ctx *c, hipStream_t st, hipEvent_t ev)
{
  const int i = planes_slot(c, st);
  for (int j = 0; j < 4; j++) if (j != i && c->st.planes_ev[j] == ev) c->st.planes_ev[j] = nullptr;
  if (c->st.planes_busy[i]) c->st.planes_ev[i] = ev;
}
inline void planes_idle(uvaia_gpu_ctx *c, bool main, bool scans)
{ for (int i = 0; i < 4; i++) if (i == 0 ? main : scans) { c->st.planes_busy[i] = false; c->st.planes_ev[i] = nullptr; } }

// a pair of timing events for one scan launch: from the pool if it has any
int take_scan_events(uvaia_gpu_ctx *c, ScanEvt &ev)
{
  for (Event *e : {&ev.a, &ev.b}) {
    if (!c->stats.ev_pool.empty()) { *e = std::move(c->stats.ev_pool.back()); c->stats.ev_pool.pop_back(); }
    else if (int rc = e->make(c)) return rc;
  }
  return 0;
}

int launch_scan(uvaia_gpu_ctx *c, const TileStore &s, long long tile_first, int n_tiles, const uint32_t *qp, int n_rows, int4 *out, int ppad, double bytes)
{
  if (n_tiles <= 0) return 0;
  dim3 grid((unsigned)((n_rows + c->qt - 1) / c->qt), (unsigned)((n_tiles + 3) / 4)), block(256);   // only tiles holding real queries
  ScanEvt ev{};
  if (c->stats.profile) {
    { int rc_ = take_scan_events(c, ev); if (rc_) return rc_; }
    HIPCHK(c, hipEventRecord(ev.a, c->st.stream));
  }
#define LAUNCH(K, QT) hipLaunchKernelGGL((K<QT>), grid, block, 0, c->st.stream, s.planes, tile_first, n_tiles, c->W4, qp, out, ppad)
  if (c->acgt) { switch (c->qt) { case 8: LAUNCH(scan_acgt_kernel, 8); break; case 32: LAUNCH(scan_acgt_kernel, 32); break; default: LAUNCH(scan_acgt_kernel, 16); } }
  else         { switch (c->qt) { case 8: LAUNCH(scan_iupac_kernel, 8); break; case 32: LAUNCH(scan_iupac_kernel, 32); break; default: LAUNCH(scan_iupac_kernel, 16); } }
#undef LAUNCH
  HIPCHK(c, hipGetLastError());
  if (c->stats.profile) { HIPCHK(c, hipEventRecord(ev.b, c->st.stream)); ev.bytes = bytes; c->stats.evts.push_back(std::move(ev)); }
  return 0;
}

// text - ACGT matches and partial - text matches of every pair of the slice, next to the column-compressed scan (pair_extras_kernel)
int launch_pair_extras(uvaia_gpu_ctx *c, const TileStore &s, long long tile_first, int n_tiles, uint32_t *ext, int ppad, hipStream_t stream)
{
  if (n_tiles <= 0) return 0;
  hipLaunchKernelGGL(pair_extras_kernel, dim3((unsigned)n_tiles, (unsigned)((c->nq + 15) / 16)), dim3(256), 0, stream, s.planes, tile_first, n_tiles, c->W4,
                     s.amb, c->tab.d_qp, c->tab.d_amb_q, c->nq, ext, ppad);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// rt (nullable unless the query set has constant-and-complete columns): the untruncated consensus pre-score of the slice's references,
// by the packed-plane scans themselves or, next to the column-compressed scan, by consensus_rt_kernel on the same stream
int launch_scan2(uvaia_gpu_ctx *c, const TileStore &s, long long tile_first, int n_tiles, uint32_t *out, int ppad, double bytes, hipStream_t stream,
                 int2 *tmin, int r_lo, int r_hi, int4 *rt, uint32_t *ext = nullptr /* default mode, packed-plane scan: the other two counters of every pair */, uint32_t *rtp = nullptr, uint4 *tb8 = nullptr)
{
  if (n_tiles <= 0) return 0;
  if (!stream) stream = c->st.stream;
  const bool cons = c->n_idx_c > 0;
  if (cons && !rt) return fail(c, UVAIA_GPU_ESTATE, "no buffer for the consensus pre-score");
  const uint4 *tiles = s.planes; const int *tot_tile0 = s.tot + tile_first * 64;
  const long long ptile_first = tile_first;       // packed tiles (tile_first may be renumbered for the derived planes below)
  auto consensus_rt = [&]() {
    if (!cons) return;
    if (c->acgt) hipLaunchKernelGGL((consensus_rt_kernel<true>), dim3((n_tiles + 3) / 4), dim3(256), 0, stream, tiles, ptile_first, n_tiles, c->W4, c->tab.d_cp, rt);
    else         hipLaunchKernelGGL((consensus_rt_kernel<false>), dim3((n_tiles + 3) / 4), dim3(256), 0, stream, tiles, ptile_first, n_tiles, c->W4, c->tab.d_cp, rt);
  };
  // Query tile of the packed-plane scans (their partial sums share LDS: no 32).  With eight queries counted per plane word the
  // kernel's VALU time equals its HBM time; a set of one, two or four queries is not padded to eight: the counting shrinks with it
  // and the scan stays bound by HBM (DESIGN.md 4.1).
  const int qt2 = c->qt != 8 ? 16 : c->nq <= 1 ? 1 : c->nq <= 2 ? 2 : c->nq <= 4 ? 4 : 8;
  const int n_qtiles = (c->nq + qt2 - 1) / qt2;
  dim3 grid(scan_grid_size(n_qtiles, n_tiles)), block(256);      // the packed-plane scans: one block per (query tile, tile of references)
  ScanEvt ev_{};
  if (c->stats.profile) {
    { int rc_ = take_scan_events(c, ev_); if (rc_) return rc_; }
    HIPCHK(c, hipEventRecord(ev_.a, stream));
  }
  const uint32_t *qp = c->acgt ? c->tab.d_qp : c->tab.d_qp2;
  if (c->scan_variant == 2) {
    planes_touch(c, stream);
    const int *tote = s.tote + tile_first * 64;
    constexpr int QS = 64;                       // queries of a super-tile of scan3_kernel
    if (c->act_q0 % QS) return fail(c, UVAIA_GPU_ESTATE, "the scan works on super-tiles of %d queries: active queries start at a multiple of that", QS);
    const int st_first = c->act_q0 / QS, n_st = (c->act_q1 + QS - 1) / QS - st_first;
    const int R = c->scan_R;
    dim3 grid3(scan_grid_size(n_st, (n_tiles + R - 1) / R));
#define SCAN3_LAUNCH(NWW, A, RR) hipLaunchKernelGGL((scan3_kernel<NWW, A, RR>), grid3, dim3(64 * NWW), 0, stream, s.ev, s.poly, tile_first, n_tiles, c->W4, c->tab.NP4, c->tab.NP4 + c->tab.NR4, c->tab.d_qpl, c->tab.d_stream, c->tab.d_sdir, s.grp, tote, tot_tile0, out, ppad, n_st, tmin, r_lo, r_hi, st_first)
#define SCAN3_NW(A, RR) { if (c->scan_NW == 8) SCAN3_LAUNCH(8, A, RR); else SCAN3_LAUNCH(4, A, RR); }
    if (R == 4)      { if (c->acgt) SCAN3_LAUNCH(8, true, 4); else SCAN3_LAUNCH(8, false, 4); }     // four tiles per wave: eight waves only (open_tuned)
    else if (R == 2) { if (c->acgt) SCAN3_NW(true, 2) else SCAN3_NW(false, 2) }
    else             { if (c->acgt) SCAN3_NW(true, 1) else SCAN3_NW(false, 1) }
#undef SCAN3_NW
#undef SCAN3_LAUNCH
    HIPCHK(c, hipGetLastError());
    if (c->stats.profile) { HIPCHK(c, hipEventRecord(ev_.b, stream)); ev_.bytes = bytes; c->stats.evts.push_back(std::move(ev_)); }
    consensus_rt();
    HIPCHK(c, hipGetLastError());
    if (tb8 && !c->acgt) {     // 33-128 queries, default mode: the sharp bounds replay3_kernel walks (the other two counters of every pair: launch_pair_extras)
      hipLaunchKernelGGL(tile_bounds_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, out, ppad, n_tiles, c->nq, r_lo, r_hi, tb8, cons ? rt : (const int4 *)nullptr, rtp);
      HIPCHK(c, hipGetLastError());
      if (ext) { int rc_ = launch_pair_extras(c, s, ptile_first, n_tiles, ext, ppad, stream); if (rc_) return rc_; }
    }
    return 0;
  }
  const int *amb0 = s.amb;       // side rows of tile 0 of the store
#define LAUNCH(K, QT, CN) hipLaunchKernelGGL((K<QT, CN>), grid, block, 0, stream, tiles, tile_first, n_tiles, c->W4, qp, out, ppad, n_qtiles, tot_tile0, tmin, r_lo, r_hi, c->tab.d_cp, rt)
#define LAUNCHX(K, QT, CN) hipLaunchKernelGGL((K<QT, CN>), grid, block, 0, stream, tiles, tile_first, n_tiles, c->W4, qp, out, ppad, n_qtiles, tot_tile0, tmin, r_lo, r_hi, c->tab.d_cp, rt, ext, rtp, tb8, amb0, c->tab.d_qp, c->tab.d_amb_q, c->nq)
#define LAUNCH_QT(L, K, CN) switch (qt2) { case 1: L(K, 1, CN); break; case 2: L(K, 2, CN); break; case 4: L(K, 4, CN); break; case 8: L(K, 8, CN); break; default: L(K, 16, CN); }
  if (c->acgt) { if (cons) { LAUNCH_QT(LAUNCH, scan2_acgt_kernel, true) } else { LAUNCH_QT(LAUNCH, scan2_acgt_kernel, false) } }
  else         { if (cons) { LAUNCH_QT(LAUNCHX, scan2_iupac_kernel, true) } else { LAUNCH_QT(LAUNCHX, scan2_iupac_kernel, false) } }
#undef LAUNCH_QT
#undef LAUNCHX
#undef LAUNCH
  HIPCHK(c, hipGetLastError());
  if (c->stats.profile) { HIPCHK(c, hipEventRecord(ev_.b, stream)); ev_.bytes = bytes; c->stats.evts.push_back(std::move(ev_)); }
  return 0;
}

// dynamic LDS of replay3_kernel: the heap, the bitmap of the query's listed words, the ring of 16 rounds of tile bounds (1 KB each), two
// staging buffers of 32, 16 or 8 tiles (the context's staging depth) x 3 (4 with a consensus pre-score) arrays x 64 dwords
size_t replay3_lds_bytes(const uvaia_gpu_ctx *c)
{ return (size_t)(c->k + 1) * HEAP_ENTRY * sizeof(int) + 128 + (size_t)16 * 1024 + (size_t)2 * c->replay_half * (c->n_idx_c > 0 ? 4 : 3) * 256; }
int ensure_cnt4(uvaia_gpu_ctx *c, size_t elems) { return c->state.d_cnt.reserve(c, elems); }

int collect_events(uvaia_gpu_ctx *c)
{
  for (auto &e : c->stats.evts) {
    HIPCHK(c, hipEventSynchronize(e.b));
    float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, e.a, e.b));
    c->stats.scan_ms += ms; c->stats.scan_bytes += e.bytes; c->stats.scan_launches++;
    c->stats.ev_pool.push_back(std::move(e.a)); c->stats.ev_pool.push_back(std::move(e.b));
  }
  c->stats.evts.clear();
  return 0;
}

// One launch of the gate/heap replay over a scanned range: queries [q0, q1), one block each, over references rb .. re-1 (relative to
// tile tile_first of `planes`).  The context decides the kernel: the four-counter replay (fullscan: counters, pre-score and entered
// rows in d_cnt / d_rt / d_tr), replay3_kernel where the scan left the extras (ext), else replay2_kernel with its on-demand counters.
struct ReplayLaunch {
  hipStream_t stream; int q0, q1;
  const uint32_t *cnt, *ext; int ppad; const int4 *rt; const uint32_t *rtp; const int2 *tmin; const uint4 *tb8;
  const uint4 *planes; long long tile_first; const int *nonn, *amb; uint8_t *entered;
  int rb, re; long long ord_base;
  const uint32_t *qpl; const uint4 *poly; int nr4; const uint32_t *qrare;   // on-demand counters from the planes derived for the query set (null, 0: from the packed ones)
  int prefetch;                                                             // candidates of a tile whose on-demand counters are requested ahead: 1, 2 or 3
};
// the regime replay2_lean_kernel is written for, as far as the context decides it (launch_replay adds what a launch decides)
static bool lean_replay_context(const uvaia_gpu_ctx *c) { return !c->fullscan && !c->use_ext && !c->acgt && c->n_idx_c == 0 && c->k <= 127; }
int launch_replay(uvaia_gpu_ctx *c, const ReplayLaunch &L)
{
  const dim3 grid(L.q1 - L.q0), block(64);
  const size_t lds = (size_t)(c->k + 1) * HEAP_ENTRY * sizeof(int);
  c->state.entered_clean = 0;                      // every replay sets entered flags
  if (L.poly) planes_touch(c, L.stream);     // (on-demand counters from the derived planes)
  if (c->fullscan) {
#define REPLAY(A) hipLaunchKernelGGL((replay_kernel<A>), grid, block, lds, L.stream, c->state.d_cnt, L.ppad, c->state.d_rt, c->state.d_tr, L.nonn, L.rb, L.re, L.ord_base, c->state.d_heap, c->state.d_n, c->state.d_T, c->state.d_snap, L.entered, c->k)
    if (c->acgt) REPLAY(true); else REPLAY(false);
#undef REPLAY
  } else if (L.ext) {     // the scan left every counter of every pair: the replay without a round trip per admission, with the context's staging depth
#define REPLAY3(B, H) hipLaunchKernelGGL((replay3_kernel<B, H>), grid, block, replay3_lds_bytes(c), L.stream, L.cnt, L.ext, L.ppad, L.rt, L.rtp, c->tab.d_cp, L.nonn, L.amb, L.rb, L.re, L.ord_base, \
                                         c->state.d_heap, c->state.d_n, c->state.d_T, c->state.d_snap, L.entered, c->k, L.planes, L.tile_first, c->W4, c->tab.d_qp, c->tab.d_amb_q, c->stats.d_stats, L.q0, L.tb8, c->replay_prio)
#define REPLAY3_HALF(B) { if (c->replay_half == 32) REPLAY3(B, 32); else if (c->replay_half == 16) REPLAY3(B, 16); else REPLAY3(B, 8); }
    if (c->n_idx_c > 0) REPLAY3_HALF(true) else REPLAY3_HALF(false)
#undef REPLAY3_HALF
#undef REPLAY3
  } else {
    const int lq_words = (c->replay_lq && !c->acgt && lds + (size_t)c->W4 * 4 * 6 * 4 + 128 <= 64 * 1024) ? c->W4 * 4 * 6 : 0;   // query planes cached in LDS
#define REPLAY2(A, B, PF_) hipLaunchKernelGGL((replay2_kernel<A, B, PF_>), grid, block, lds + (size_t)lq_words * 4 + 128, L.stream, L.cnt, L.ppad, L.rt, c->tab.d_cp, L.nonn, L.amb, L.rb, L.re, L.ord_base, \
                                              c->state.d_heap, c->state.d_n, c->state.d_T, c->state.d_snap, L.entered, c->k, L.planes, L.tile_first, c->W4, c->tab.d_qp, c->tab.d_amb_q, c->stats.d_stats, L.q0, L.tmin, L.qpl, lq_words, c->replay_prio, \
                                              L.poly, c->tab.NP4 + c->tab.NR4, c->tab.NP4, L.nr4, L.qrare)
#define REPLAY2_PF(A, B) { if (L.prefetch == 1) REPLAY2(A, B, 1); else if (L.prefetch == 2) REPLAY2(A, B, 2); else REPLAY2(A, B, 3); }
    // default mode, no consensus pre-score, two candidates requested ahead, the query's planes in memory, a lane per inner node of the
    // heap: the regime of a large query set (config[1]) has the kernel written for it (a build with -DREPLAY_TIMING keeps the one with the probes)
    bool lean = lean_replay_context(c) && L.prefetch == 2 && lq_words == 0;
#ifdef REPLAY_TIMING
    lean = false;
#endif
    if (lean) hipLaunchKernelGGL(replay2_lean_kernel, grid, block, lds + 128, L.stream, L.cnt, L.ppad, L.nonn, L.amb, L.rb, L.re, L.ord_base, c->state.d_heap, c->state.d_n, c->state.d_T, L.entered, c->k,
                                 L.planes, L.tile_first, c->W4, c->tab.d_qp, c->tab.d_amb_q, c->stats.d_stats, L.q0, L.tmin, c->replay_prio);
    else if (c->acgt) { if (c->n_idx_c > 0) REPLAY2_PF(true, true) else REPLAY2_PF(true, false) }
    else              { if (c->n_idx_c > 0) REPLAY2_PF(false, true) else REPLAY2_PF(false, false) }
#undef REPLAY2_PF
#undef REPLAY2
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// One batch = one pool of the reference (src/nearest.c:288-306), on tiles [tile_first, tile_first+n_tiles) of the store;
// references r_begin..r_end-1 (relative to the first tile) are the batch, in order.
int run_batch(uvaia_gpu_ctx *c, const TileStore &s, long long tile_first, int n_tiles, int r_begin, int r_end,
              long long ord_base)
{
  if (r_end <= r_begin) return 0;   // an empty trailing batch only refreshes cq->max_incompatible (src/nearest.c:290-291)
  const int ppad = n_tiles * 64;
  const SliceBuf &b = c->slice[0];
  hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(256), 0, c->st.stream, c->state.d_T, c->nq, c->state.d_snap);
  if (c->n_idx_c > 0 && c->fullscan) {   // with no constant-and-complete column every pre-score counter is zero (common: gappy query sets)
    if (c->acgt) hipLaunchKernelGGL((consensus_kernel<true>), dim3((n_tiles + 3) / 4), dim3(256), 0, c->st.stream, s.planes, tile_first, n_tiles, c->W4, c->tab.d_cp, c->state.d_snap, c->state.d_rt, c->state.d_tr);
    else         hipLaunchKernelGGL((consensus_kernel<false>), dim3((n_tiles + 3) / 4), dim3(256), 0, c->st.stream, s.planes, tile_first, n_tiles, c->W4, c->tab.d_cp, c->state.d_snap, c->state.d_rt, c->state.d_tr);
  }
  HIPCHK(c, hipGetLastError());
  const double bytes = (double)(r_end - r_begin) * (double)c->W4 * 16.0 * c->P + (double)c->nq * (double)c->W4 * 16.0 * c->P;
  uint32_t *ext = c->use_ext ? b.ext : nullptr;
  int rc = 0;
  if (c->fullscan) {
    rc = ensure_cnt4(c, (size_t)c->nq_pad * c->pool_pad); if (rc) return rc;
    rc = launch_scan(c, s, tile_first, n_tiles, c->tab.d_qp, c->nq, c->state.d_cnt, ppad, bytes);
  } else rc = launch_scan2(c, s, tile_first, n_tiles, b.cnt, ppad, bytes, nullptr, b.tmin, r_begin, r_end, b.rt, ext, b.rtp, b.tb8);
  if (rc) return rc;
  rc = launch_replay(c, {c->st.stream, 0, c->nq, b.cnt, ext, ppad, b.rt, b.rtp, b.tmin, b.tb8,
                             s.planes, tile_first, s.nonn + tile_first * 64, s.amb + tile_first * 64 * AMB_ROW, c->state.d_entered + tile_first * 64, r_begin, r_end, ord_base,
                             c->scan_variant == 2 ? c->tab.d_qpl : nullptr, s.poly, c->tab.NR4, c->tab.d_qrare, 3});
  if (rc) return rc;
  c->last = {&s, tile_first, n_tiles, r_end - r_begin, r_begin, ppad, c->fullscan ? c->state.d_rt : b.rt};
  return 0;
}

// planes derived for the open query set (column-compressed scan) for the whole tiles that hold slots slot0 .. slot0 + n_ref - 1 of
// the store (resident database under reference shards: the context's own numbering of the tiles it keeps, see for_owned_tiles)
int derive_rows(uvaia_gpu_ctx *c, const TileStore &s, long long slot0, int n_ref, hipStream_t st = nullptr, bool v_in_place = false)
{
  if (!st) st = c->st.stream;
  if (c->fullscan || c->scan_variant != 2 || n_ref <= 0 || !c->tab.d_split) return 0;     // only the column-compressed scan reads derived planes
  if (st == c->st.stream) planes_touch(c, st);       // (the rebuild's own streams are in order among themselves)
  const long long a = slot0 / 64, t1 = (slot0 + n_ref - 1) / 64;
  const int nblk = (int)(t1 - a + 1);
  // Waves per tile: the same arrays from every width.  Four unless tuning.derive_waves asks for 8 or 16 -- measured at config[1], one box,
  // interleaved: 2.93 / 2.96 / 2.97 ms per step with 4 / 8 / 16 everywhere, 2.92-2.95 with 16 for a rebuild's first chunk and 4 or 8 beside the
  // scans; the first chunk of 273 tiles takes 101-105 us at 4 waves and 103 at 16 (DESIGN.md 4.2: a launch of that size is not bound by a
  // wave's chain of loads).
  const int waves = c->derive_waves ? c->derive_waves : 4;
#define DERIVE_ALL_W(A, V, N) hipLaunchKernelGGL((derive_all_kernel<A, V, N>), dim3(nblk), dim3(64 * N), 0, st, s.planes, a, a, c->W4, c->tab.d_cls, c->tab.d_rmask, c->tab.d_split + derive_split_offset(N), c->tab.NP4, c->tab.NR4, s.ev, s.tote, s.grp, s.poly)
#define DERIVE_ALL(A, V) { if (waves == 8) DERIVE_ALL_W(A, V, 8); else if (waves == 16) DERIVE_ALL_W(A, V, 16); else DERIVE_ALL_W(A, V, 4); }
  if (c->acgt) { if (v_in_place) DERIVE_ALL(true, false) else DERIVE_ALL(true, true) }
  else         { if (v_in_place) DERIVE_ALL(false, false) else DERIVE_ALL(false, true) }
#undef DERIVE_ALL
#undef DERIVE_ALL_W
  HIPCHK(c, hipGetLastError());
  return 0;
}

int sync_scan_streams(uvaia_gpu_ctx *c) { for (hipStream_t st : c->st.scan_streams) if (st) HIPCHK(c, hipStreamSynchronize(st)); planes_idle(c, false, true); return 0; }
int sync_derive_streams(uvaia_gpu_ctx *c) { for (hipStream_t st : c->st.derive_streams) if (st) HIPCHK(c, hipStreamSynchronize(st)); return 0; }

// room in a counter buffer for `need` pairs of a slice of ppad columns: never less than a pool's, and never less than it held before
// (buffer 0 is the push path's too); the streams that may still use the arrays are waited for before they go
int slice_reserve(uvaia_gpu_ctx *c, SliceBuf &b, size_t need, size_t ppad)
{
  need = std::max(need, b.cnt.cap);
  if (need <= b.cnt.cap && b.tmin) return 0;
  if (int rc = sync_scan_streams(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  const size_t cap = std::max(need, (size_t)c->nq_pad * c->pool_pad), refs = std::max(cap / (size_t)c->nq_pad, ppad) + 64;
  if (int rc = b.cnt.reserve(c, cap)) return rc;
  if (int rc = b.tmin.reserve(c, cap / 64)) return rc;
  if (c->use_ext) {
    if (int rc = b.ext.reserve(c, cap)) return rc;
    if (int rc = b.tb8.reserve(c, cap / 64)) return rc;
    if (int rc = b.rtp.reserve(c, refs)) return rc;
  }
  return b.rt.reserve(c, refs);
}

// a rebuild of the derived planes still in flight (uvaia_gpu_db_rederive) must end before the database changes
static int settle_derive(uvaia_gpu_ctx *c)
{
  if (c->st.derive_pending) { if (int rc = sync_derive_streams(c)) return rc; c->st.derive_pending = 0; }
  return 0;
}

// ---- rows on their way into a store, step by step: each step is written here once, and the entries of the resident database
// (uvaia_gpu_db_append*, uvaia_gpu_db_load_staged: host_resident.inc, host_rows.inc, host_window.inc) are sequences of them

int db_refuse_full(uvaia_gpu_ctx *c) { return fail(c, UVAIA_GPU_ESTATE, "database capacity %zu exceeded: call uvaia_gpu_db_reserve first", c->db_cap); }

// room for n more references: a rebuild in flight ends first; an empty database reserves for itself, one that holds references refuses
int db_make_room(uvaia_gpu_ctx *c, size_t n)
{
  if (int rc = settle_derive(c)) return rc;
  if (c->db_n + n <= c->db_cap) return 0;
  return c->db_n ? db_refuse_full(c) : uvaia_gpu_db_reserve(c, n);
}

// pack_refs_kernel over one staged chunk: the m rows at ds become slots s0 .. s0 + m - 1 of the store; non_n (nullable): the caller's
// valid-site counts of these rows instead of the kernel's
int launch_pack_chunk(uvaia_gpu_ctx *c, const uint8_t *ds, int m, const TileStore &s, long long s0, const int *non_n)
{
  const long long t0 = s0 / 64, t1 = (s0 + m - 1) / 64;
  const int nblk = (int)(t1 - t0 + 1);
  int *nn_out = non_n ? nullptr : s.nonn.p;
  if (c->acgt) hipLaunchKernelGGL((pack_refs_kernel<3>), dim3(nblk), dim3(256), 0, c->st.stream, ds, c->pitch, c->nchar, s0, m, c->W4, s.planes, t0, nn_out, (int *)nullptr, s.tot, c->state.d_err);
  else         hipLaunchKernelGGL((pack_refs_kernel<4>), dim3(nblk), dim3(256), 0, c->st.stream, ds, c->pitch, c->nchar, s0, m, c->W4, s.planes, t0, nn_out, s.amb, s.tot, c->state.d_err);
  HIPCHK(c, hipGetLastError());
  if (non_n) HIPCHK(c, hipMemcpyAsync(s.nonn + s0, non_n, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
  return 0;
}

// the flag pack_refs_kernel raises at a byte outside the alphabet, read and cleared (the stream has been waited for)
int take_pack_error(uvaia_gpu_ctx *c)
{
  int bad = 0;
  HIPCHK(c, hipMemcpy(&bad, c->state.d_err, sizeof(int), hipMemcpyDeviceToHost));
  if (!bad) return 0;
  HIPCHK(c, hipMemset(c->state.d_err, 0, sizeof(int)));
  return fail(c, UVAIA_GPU_EALPHABET, "a reference sequence holds a byte outside ACGT / MRWSYKVHDB / NX-?O.");
}

// n_tiles tiles of the resident database from tile t0 on, out of their four-plane form: the totals and, --acgt, the three planes re-coded
// from `four`, which holds that form of those tiles (default mode: the resident planes are that form already, `four` is not read)
int db_import_tiles(uvaia_gpu_ctx *c, const uint4 *four, long long t0, size_t n_tiles)
{
  if (c->acgt) hipLaunchKernelGGL((import_tiles_kernel<3>), dim3((unsigned)n_tiles), dim3(256), 0, c->st.stream, four, c->W4, c->db.planes, t0, c->db.tot);
  else         hipLaunchKernelGGL((import_tiles_kernel<4>), dim3((unsigned)n_tiles), dim3(256), 0, c->st.stream, c->db.planes + (size_t)t0 * c->W4 * 4 * 64, c->W4, (uint4 *)nullptr, t0, c->db.tot);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// the checks on what came from outside -- valid-site counts, side rows -- for slots slot0 .. slot0 + n - 1 of the resident database
int db_sanitise_import(uvaia_gpu_ctx *c, size_t slot0, size_t n)
{
  hipLaunchKernelGGL(sanitise_import_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->st.stream, c->acgt ? (int *)nullptr : c->db.amb + slot0 * AMB_ROW, c->db.nonn + slot0,
                     (long long)n, c->W4 * 4, c->nchar);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// side rows of slots slot0 .. slot0 + n_ref - 1 of the resident database in their fixed form (side_rows_canonical_kernel: what an export, and
// with it a packed database file, holds must not depend on the timing of pack_refs_kernel's waves); wait: returns when it is done
int db_canonical_side_rows(uvaia_gpu_ctx *c, long long slot0, int n_ref, bool wait)
{
  if (c->acgt || n_ref <= 0 || !c->db.amb) return 0;
  const long long t0 = slot0 / 64, t1 = (slot0 + n_ref - 1) / 64;
  hipLaunchKernelGGL(side_rows_canonical_kernel, dim3((unsigned)(t1 - t0 + 1)), dim3(64), 0, c->st.stream, c->db.planes, c->W4, t0, slot0, n_ref, c->db.amb);
  HIPCHK(c, hipGetLastError());
  if (wait) HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

// room in the four-plane image of a window (--acgt) for `tiles` tiles, never less than the resident store holds; *grown: what it held is gone
int win_image_room(uvaia_gpu_ctx *c, size_t tiles, bool *grown)
{
  const size_t tile_u4 = (size_t)c->W4 * 4 * 64;
  if (!c->acgt || c->win.d_four.cap >= tiles * tile_u4) return 0;
  *grown = true;
  return c->win.d_four.reserve(c, std::max(tiles, c->db_cap / 64 + 1) * tile_u4);
}

// the end of an entry: the references the stream holds now, and those of them a four-plane image covers (0: rows that did not come through
// the staged calls, no image covers them)
void db_commit(uvaia_gpu_ctx *c, size_t db_n, int win_n) { c->db_n = db_n; c->win.n = win_n; c->db_gen++; }

// stage + pack n_ref rows (either scattered pointers or one pitched block) into the store starting at slot0
int pack_rows(uvaia_gpu_ctx *c, const char *const *seq, const char *rows, size_t rows_pitch, const int *non_n, int n_ref, const TileStore &s, long long slot0)
{
  // two staging buffers: while chunk k crosses PCIe and is packed, the host threads copy chunk k + 1 into the other pinned buffer
  // (the hand-over of raw characters, 30 KB per reference, is what bounds the streaming entry points, not the kernels)
  for (int done = 0, k = 0; done < n_ref; done += PACK_CHUNK, k ^= 1) {
    const int m = std::min(PACK_CHUNK, n_ref - done);
    if (c->stage_busy[k]) { HIPCHK(c, hipEventSynchronize(c->stage_free[k])); c->stage_busy[k] = false; }     // its previous chunk has left the buffer
    uint8_t *hs = c->h_stage + (size_t)k * PACK_CHUNK * c->pitch, *ds = c->d_stage + (size_t)k * PACK_CHUNK * c->pitch;
    for (int i = 0; i < m; i++) if (!(seq ? seq[done + i] : rows)) return fail(c, UVAIA_GPU_EINVAL, "NULL sequence at position %d", done + i);
    parallel_for(m, [&](int i) {
      const char *src = seq ? seq[done + i] : rows + (size_t)(done + i) * rows_pitch;
      memcpy(hs + (size_t)i * c->pitch, src, (size_t)c->nchar);
    });
    HIPCHK(c, hipMemcpyAsync(ds, hs, (size_t)m * c->pitch, hipMemcpyHostToDevice, c->st.stream));
    if (int rc = launch_pack_chunk(c, ds, m, s, slot0 + done, non_n ? non_n + done : nullptr)) return rc;
    HIPCHK(c, hipEventRecord(c->stage_free[k], c->st.stream)); c->stage_busy[k] = true;
  }
  { int rc = derive_rows(c, s, slot0, n_ref); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));     // scans may start on another stream: the packed and derived planes must be complete
  planes_idle(c, true, false);
  return take_pack_error(c);
}

}  // namespace
