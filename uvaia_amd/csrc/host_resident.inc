// host_resident.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the HBM-resident database: appends, packed interchange form, derived planes, sub-sliced search, slices and state for several GPUs, introspection.

extern "C" {

int uvaia_gpu_db_reserve(uvaia_gpu_ctx *c, size_t cap)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (cap <= c->db_cap) return 0;
  if (c->db_n) return fail(c, UVAIA_GPU_ESTATE, "reserve the database before appending to it");
  const size_t tiles = (cap + 63) / 64 + 1;
  // reference shards: everything that is kept per reference -- packed planes, side rows, counts, derived planes -- for the owned pieces
  // only (+ one tile: a piece may end inside the capacity's last tile)
  const size_t dtiles = derived_tiles(c, tiles) + (c->shard.world > 1 ? 1 : 0);
  if (int rc = store_alloc(c, c->db, dtiles)) return rc;
  c->db_local_tiles = dtiles;
  c->shard.peer_db[c->shard.rank] = c->db.planes; c->shard.peer_amb[c->shard.rank] = c->db.amb;
  c->db_cap = tiles * 64 - 64;
  c->state.entered_clean = 0;
  if (int rc = c->state.d_entered.reserve(c, tiles * 64)) return rc;
  HIPCHK(c, hipMemset(c->state.d_entered, 0, c->state.d_entered.cap));
  HIPCHK(c, hipStreamSynchronize(nullptr));             // (as in store_alloc: the flags are zero before a search on another stream sets them)
  return 0;
}

static int db_append_common(uvaia_gpu_ctx *c, const char *const *seq, const char *rows, size_t pitch, const int *non_n, int n_ref)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_ref < 0) return fail(c, UVAIA_GPU_EINVAL, "negative count");
  if (n_ref == 0) return 0;
  if (int rc = db_make_room(c, (size_t)n_ref)) return rc;
  // reference shards: the caller hands every context the whole stream; a context stages, packs and keeps the references of its own
  // pieces (local slot = local tile * 64 + position in the tile) and only counts the others
  const long long s0 = (long long)c->db_n, s1 = s0 + n_ref;
  for (long long a = s0; a < s1;) {
    const long long pe = c->shard.world == 1 ? s1 : std::min(s1, (a / (c->shard.pt * 64) + 1) * c->shard.pt * 64);
    if (owns_tile(c, a / 64)) {
      const long long off = a - s0, local = dtile_of(c, a / 64) * 64 + a % 64;
      int rc = pack_rows(c, seq ? seq + off : nullptr, rows ? rows + (size_t)off * pitch : nullptr, pitch, non_n ? non_n + off : nullptr, (int)(pe - a), c->db, local);
      if (rc) return rc;
      rc = db_canonical_side_rows(c, local, (int)(pe - a), true);
      if (rc) return rc;
    }
    a = pe;
  }
  db_commit(c, c->db_n + (size_t)n_ref, 0);
  return 0;
}

int uvaia_gpu_db_skip(uvaia_gpu_ctx *c, size_t n_ref)
{ // the next n_ref references of the stream belong to other ranks' pieces: nothing to keep, the stream position moves on
  if (!c) return UVAIA_GPU_EINVAL;
  if (!n_ref) return 0;
  if (c->db_n + n_ref > c->db_cap) return db_refuse_full(c);
  for (size_t a = c->db_n; a < c->db_n + n_ref; a = (a / 64 + 1) * 64)
    if (owns_tile(c, (long long)(a / 64))) return fail(c, UVAIA_GPU_EINVAL, "reference %zu belongs to a piece of this context: it cannot be skipped", a);
  c->db_n += n_ref; c->db_gen++;
  return 0;
}

int uvaia_gpu_db_append(uvaia_gpu_ctx *c, const char *const *seq, const int *non_n, int n_ref)
{ if (c && n_ref > 0 && !seq) return fail(c, UVAIA_GPU_EINVAL, "NULL seq"); return db_append_common(c, seq, nullptr, 0, non_n, n_ref); }

int uvaia_gpu_db_append_block(uvaia_gpu_ctx *c, const char *rows, size_t pitch, const int *non_n, int n_ref)
{
  if (c && n_ref > 0 && (!rows || pitch < (size_t)c->nchar)) return fail(c, UVAIA_GPU_EINVAL, "bad block");
  return db_append_common(c, nullptr, rows, pitch, non_n, n_ref);
}

size_t uvaia_gpu_db_size(const uvaia_gpu_ctx *c) { return c ? c->db_n : 0; }

int uvaia_gpu_db_clear(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  c->win.n = 0;                                        // the four-plane image of a loaded window goes with the rows
  c->db_gen++;
  if (!c->db.planes || !c->db_n) { c->db_n = 0; return 0; }
  { int rc = settle_derive(c); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (int rc = sync_scan_streams(c)) return rc;
  const size_t tiles = c->shard.world == 1 ? (c->db_n + 63) / 64 : c->db_local_tiles;       // lanes past the last reference of a tile must read as zero planes
  HIPCHK(c, hipMemsetAsync(c->db.planes, 0, tiles * (size_t)c->W4 * c->P * 64 * sizeof(uint4), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.nonn, 0, tiles * 64 * sizeof(int), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.tot, 0, tiles * 64 * sizeof(int), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.amb, 0, tiles * 64 * AMB_ROW * sizeof(int), c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  c->db_n = 0;
  return 0;
}

size_t uvaia_gpu_db_tile_bytes(const uvaia_gpu_ctx *c) { return c ? (size_t)c->W4 * 4 * 64 * sizeof(uint4) : 0; }
int uvaia_gpu_db_side_row_ints(void) { return AMB_ROW; }

int uvaia_gpu_db_export(uvaia_gpu_ctx *c, size_t first_tile, size_t n_tiles, void *planes, int *non_n, int *side_rows)
{
  if (!c || !planes || !non_n || !side_rows) return UVAIA_GPU_EINVAL;
  if (c->acgt) return fail(c, UVAIA_GPU_ESTATE, "the interchange form is the four IUPAC planes: export from a default-mode context");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard holds its own pieces only: export from a plain context");
  if ((first_tile + n_tiles) * 64 > ((c->db_n + 63) / 64) * 64) return fail(c, UVAIA_GPU_EINVAL, "tiles %zu..%zu lie outside the database", first_tile, first_tile + n_tiles);
  if (!n_tiles) return 0;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  const size_t tb = uvaia_gpu_db_tile_bytes(c);
  HIPCHK(c, hipMemcpy(planes, reinterpret_cast<const char *>(c->db.planes.p) + first_tile * tb, n_tiles * tb, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(non_n, c->db.nonn + first_tile * 64, n_tiles * 64 * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(side_rows, c->db.amb + first_tile * 64 * AMB_ROW, n_tiles * 64 * AMB_ROW * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int uvaia_gpu_db_derived_export(uvaia_gpu_ctx *c, size_t n_tiles, void *e, uint32_t *grp, void *poly, int *tot)
{ // introspection: what derive_all_kernel left for the first n_tiles tiles, after any rebuild in flight
  if (!c || !e || !grp || !poly || !tot) return UVAIA_GPU_EINVAL;
  if (c->fullscan || c->scan_variant != 2 || !c->db.ev) return fail(c, UVAIA_GPU_ESTATE, "only the column-compressed scan keeps planes derived for the query set");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard numbers its derived tiles by piece: read them from a plain context");
  if (n_tiles * 64 > ((c->db_n + 63) / 64) * 64) return fail(c, UVAIA_GPU_EINVAL, "tiles 0..%zu lie outside the database", n_tiles);
  if (!n_tiles) return 0;
  { int rc = settle_derive(c); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  const size_t W4 = (size_t)c->W4, NG = (size_t)(c->tab.NP4 + c->tab.NR4);
  HIPCHK(c, hipMemcpy2D(e, 1024, c->db.ev, 2048, 1024, n_tiles * W4, hipMemcpyDeviceToHost));        // [tile][w4][E, V][64] uint4: the E halves
  HIPCHK(c, hipMemcpy(grp, c->db.grp, n_tiles * W4 * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (NG) HIPCHK(c, hipMemcpy(poly, c->db.poly, n_tiles * NG * 3 * 64 * sizeof(uint4), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(tot, c->db.tote, n_tiles * 64 * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int uvaia_gpu_db_append_packed(uvaia_gpu_ctx *c, const void *planes, const int *non_n, const int *side_rows, int n_ref)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_ref < 0) return fail(c, UVAIA_GPU_EINVAL, "negative count");
  if (n_ref == 0) return 0;
  if (!planes || !non_n || (!c->acgt && !side_rows)) return fail(c, UVAIA_GPU_EINVAL, "NULL packed arrays");
  if (c->db_n % 64) return fail(c, UVAIA_GPU_ESTATE, "packed tiles can only follow a whole number of tiles (database holds %zu references)", c->db_n);
  if (int rc = db_make_room(c, (size_t)n_ref)) return rc;
  const size_t tb = uvaia_gpu_db_tile_bytes(c), n_tiles_all = ((size_t)n_ref + 63) / 64;
  const long long t0g = (long long)(c->db_n / 64);
  // (reference shards: only the tiles of the context's own pieces are copied in, under their local numbers)
  int rc = for_owned_tiles(c, t0g, t0g + (long long)n_tiles_all, [&](long long gt, long long t0, long long nt) -> int {
    const size_t n_tiles = (size_t)nt, off = (size_t)(gt - t0g);
    const char *pl = reinterpret_cast<const char *>(planes) + off * tb;
    if (!c->acgt) {     // same form as the resident planes: straight into place, then the totals
      HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char *>(c->db.planes.p) + (size_t)t0 * tb, pl, n_tiles * tb, hipMemcpyHostToDevice, c->st.stream));
      if (int rc = db_import_tiles(c, nullptr, t0, n_tiles)) return rc;
      HIPCHK(c, hipMemcpyAsync(c->db.amb + (size_t)t0 * 64 * AMB_ROW, side_rows + off * 64 * AMB_ROW, n_tiles * 64 * AMB_ROW * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
    } else {            // re-code through a staging buffer, a few tiles at a time
      const size_t chunk = 64;
      DevBuf<uint4> d_tmp;
      if (int rc = d_tmp.reserve(c, chunk * tb / sizeof(uint4))) return rc;
      for (size_t a = 0; a < n_tiles; a += chunk) {
        const size_t m = std::min(chunk, n_tiles - a);
        HIPCHK(c, hipMemcpyAsync(d_tmp, pl + a * tb, m * tb, hipMemcpyHostToDevice, c->st.stream));
        if (int rc = db_import_tiles(c, d_tmp, t0 + (long long)a, m)) return rc;
        HIPCHK(c, hipStreamSynchronize(c->st.stream));
      }
    }
    HIPCHK(c, hipMemcpyAsync(c->db.nonn + (size_t)t0 * 64, non_n + off * 64, n_tiles * 64 * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
    if (int rc = db_sanitise_import(c, (size_t)t0 * 64, n_tiles * 64)) return rc;
    return derive_rows(c, c->db, t0 * 64, (int)(n_tiles * 64));
  });
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  db_commit(c, c->db_n + (size_t)n_ref, 0);
  return 0;
}

// Sub-slices of the pools that tile [first, first + n): {first reference, length, opens a pool}.  A pool boundary only retakes
// the snapshot of the tolerances (src/nearest.c:290-291), which happens at a pool's first sub-slice, so cutting pools is exact.
struct SubSlice { size_t first, n; bool pool_start; };
#ifndef HEAD_TAIL_NQT
#define HEAD_TAIL_NQT 17           // query tiles below which a long pool gets a short head and a short tail slice (A/B switch)
#endif
static std::vector<SubSlice> plan_subslices(const uvaia_gpu_ctx *c, size_t first, size_t n, size_t pool)
{
  std::vector<SubSlice> subs;
  // with few queries the replay is negligible and small launches only cost: one slice per pool then.  The sub-slice length is
  // tuned for 63 query tiles (1 000 queries); with fewer active tiles (query shards) it grows so that a launch still fills the chip
  const int nqt = (c->act_q1 + 15) / 16 - c->act_q0 / 16;
  // Pool boundaries act through the snapshot only, and the snapshot only through the consensus counters: without constant-and-
  // complete query columns (n_idx_c == 0) they have no effect at all and the slices are laid over the whole range.
  if (c->n_idx_c == 0) pool = std::max<size_t>(n, 1);
  size_t sub = c->subslice;
  // With at most half the benchmark's query tiles (query shards, smaller query sets) the rebuild of the derived planes weighs
  // more against the scan: slices of half the waves let the first scan start earlier and hide more of it (measured with the
  // rebuild inside the step: 6.18 -> 6.03, 7.24 -> 7.10, 9.89 -> 9.26 ms for rank 0 of 2, 4, 8 query shards; 63 tiles: worse).
  if (nqt <= 32) sub /= 2;
  if (nqt < 63) sub = std::min(pool, (sub * 63 / (size_t)std::max(nqt, 1) + 63) / 64 * 64);
  // At most three query tiles: the scan is bound by HBM and the replay has a handful of waves; what pays is running the replay
  // of one slice next to the scan of the following ones (the pre-score no longer waits for the batch snapshot: DESIGN.md 2.3):
  // four slices per pool, none below 65 536 references.
  if (nqt < 4) sub = std::min(pool, std::max<size_t>(65536, ((pool + 3) / 4 + 63) / 64 * 64));
  if (c->subslice_forced) sub = std::min(pool, c->subslice);
  for (size_t a = first; a < first + n; a += pool) {
    const size_t pe = std::min(first + n, a + pool);
    if (nqt < HEAD_TAIL_NQT && !c->subslice_forced && pe - a >= 8 * 65536) {
      // (Up to 256 queries: measured per 1 M references with the rule up to 3 / 8 / 16 query tiles -- 64 queries 8.87-9.13 / 8.65-8.67 /
      // 8.54-8.81 ms per step, 128 queries 9.17 / 8.98-9.01 / 8.83-9.13, 256 queries 11.4-11.5 / 11.3-12.4 / 11.0-11.1.)
      // Few queries, a long pool: the replay of a pool's FIRST references is the expensive one (the heaps fill and turn over fast,
      // every admission a dependent round trip to memory for a handful of waves) and the replay of its LAST slice is exposed.  A
      // short head lets the first start early, next to the scans of the rest; a short tail keeps the exposed part small.
      // (round 4: the replays keep up with the scans now, and what a step waits for after its last scan is the replay of the LAST BUT ONE
      // slice plus the last one's: with three query tiles or fewer the slice before the tail is 131 072 references, not a full share)
      const size_t head = 65536, tail = 65536, pre = (nqt < 4 && pe - a >= 12 * 65536) ? 131072 : 0, mid = pe - a - head - tail - pre, nm = std::max<size_t>(1, (mid + sub / 2) / sub);
      const size_t each = ((mid + nm - 1) / nm + 63) / 64 * 64;
      subs.push_back({a, head, true});
      for (size_t x = a + head; x < pe - tail - pre; x += each) subs.push_back({x, std::min(each, pe - tail - pre - x), false});
      if (pre) subs.push_back({pe - tail - pre, pre, false});
      subs.push_back({pe - tail, tail, false});
      continue;
    }
    // near-equal slices (multiples of 64), as many as the pool holds sub-slice lengths, rounded: a pool of 1.05 sub-slices is
    // one launch, not a full one plus a sliver whose launch latency and replay would sit on the critical path
    const size_t len = pe - a, ns = std::max<size_t>(1, (len + sub / 2) / sub);
    const size_t each = ((len + ns - 1) / ns + 63) / 64 * 64;
    // A pool's first slice was 70 % of an equal share from round 4 on (and is where tuning.scan_streams asks for a share): the first replay -- the heaps filling and turning over, the longest of the chain of
    // replays, which ends a step at config[1] -- starts that much earlier, and so does the first scan after a rebuild of the derived planes
    // (round 4, one box, interleaved twice: 3.16 ms per step with equal slices, 3.14-3.16 / 3.00-3.07 / 3.07 with 50 / 65 / 80 %; again
    // behind the asynchronous reset and the unfenced rebuild, interleaved three times: 2.944 / 2.887 / 2.918 / 2.928 with 50 / 65 / 70 / 80 %,
    // the same configuration run twice 2.918 and 2.951 -- no difference to tell from that: 70 % stays).
    // With replay2_lean_kernel the chain of replays has slack at config[1] (its third replay ends 0.22 ms before the last scan does) and the
    // scans are the step: a short first slice only makes their launches less even.  Interleaved three times, 50 / 60 / 70 / 80 / 90 % and
    // equal slices: 2.726 / 2.724 / 2.722 / 2.701 / 2.675 / 2.669 ms per step (medians; the parent's spread over five runs is 0.028) -- equal
    // slices are the default where that kernel runs (elsewhere the 70 % stays: nothing measured there speaks for a change -- config[2], --acgt,
    // with equal slices 200.4 against 199.8 ms per step, inside the parent's spread of 1.4), and the share stays a tuning value.
    const int first_pct = c->first_slice_pct >= 0 ? c->first_slice_pct : ((lean_replay_context(c) && c->replay_lq == 0) ? 0 : 70);
    if (first_pct > 0 && first_pct < 100 && ns >= 3 && !c->subslice_forced) {
      const size_t first_n = std::max<size_t>(64, each * (size_t)first_pct / 100 / 64 * 64), rest = len - first_n;
      const size_t each2 = ((rest + (ns - 1) - 1) / (ns - 1) + 63) / 64 * 64;
      subs.push_back({a, first_n, true});
      for (size_t x = a + first_n; x < pe; x += each2) subs.push_back({x, std::min(each2, pe - x), false});
      continue;
    }
    for (size_t x = a; x < pe; x += each) subs.push_back({x, std::min(each, pe - x), x == a});
  }
  return subs;
}

int uvaia_gpu_search_plan(uvaia_gpu_ctx *c, size_t first, size_t n, size_t pool, size_t *slice_first, size_t *slice_n, unsigned char *pool_start, int cap)
{ // introspection: plan_subslices as the searches and the rebuild call it
  if (!c || cap < 0 || (cap > 0 && (!slice_first || !slice_n || !pool_start))) return UVAIA_GPU_EINVAL;
  if (pool < 1 || pool > c->max_pool) return fail(c, UVAIA_GPU_EINVAL, "pool must be in [1, max_pool=%zu]", c->max_pool);
  const std::vector<SubSlice> plan = plan_subslices(c, first, n, pool);
  if (plan.size() > (size_t)0x7fffffff) return fail(c, UVAIA_GPU_EINVAL, "a plan of %zu slices", plan.size());
  for (size_t i = 0; i < plan.size() && i < (size_t)cap; i++) { slice_first[i] = plan[i].first; slice_n[i] = plan[i].n; pool_start[i] = plan[i].pool_start ? 1 : 0; }
  return (int)plan.size();
}

int uvaia_gpu_db_rederive(uvaia_gpu_ctx *c)
{ // the reference-side work a query set costs on a database that is already resident: E/V/grp planes and gathered columns of
  // every tile for the open query set.  Appends do this for the rows they add; a caller that times "one search of a resident
  // database" without its appends calls this first so that the figure holds everything that depends on the query set.
  // Issued on its own stream in the chunks the search will scan, one event each: the first slice's scan starts as soon as its
  // chunk is done and the rest is rebuilt next to it (the rebuild is bound by HBM, the scan by instruction issue).
  if (!c) return UVAIA_GPU_EINVAL;
  if (!c->db.planes || !c->db_n || c->fullscan || c->scan_variant != 2) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<SubSlice> plan;
  if (c->shard.world == 1) plan = plan_subslices(c, 0, c->db_n, c->max_pool);
  else {   // reference shards: the chunks are the context's own pieces, which is what it scans (uvaia_gpu_shard_scan)
    const size_t piece = (size_t)c->shard.pt * 64;
    for (size_t a = (size_t)c->shard.rank * piece; a < c->db_n; a += piece * (size_t)c->shard.world) plan.push_back({a, std::min(piece, c->db_n - a), false});
  }
  // Chunks over several streams are all in flight at once: the rebuild as a whole ends sooner, its FIRST chunk -- what the first scan
  // waits for -- later.  That pays for up to three chunks; from four on -- config[1] since its first slice is 70 % of a share, and every
  // long stream -- the rebuild runs in order on one stream (1 M references: 64 queries 9.25 -> 8.65 ms per search, 256 queries 12.7 -> 11.4;
  // config[1], four chunks forced onto 1 / 2 / 3 streams, interleaved three times: 2.951 / 2.959 / 2.992 ms per step).
  const int n_derive_streams = (c->st.derive_forced || plan.size() <= 3) ? c->st.derive_nstreams : 1;
  // Searches still in flight read the planes (and an append may be writing them): the streams the rebuild uses queue behind them.  A
  // stream the host has waited for since the last such work holds nothing to wait for -- after uvaia_gpu_sync none does, and the first
  // chunk below is the call's first runtime call that reaches the device; a busy one is waited for through the event the search left
  // behind its last scan or replay, or through a record of the rebuild's own where there is none.
  {
    hipStream_t busy[4] = {c->st.stream, c->st.scan_streams[0], c->st.scan_streams[1], c->st.scan_streams[2]};
    for (int i = 0; i < 4; i++) {
      if (!busy[i] || !c->st.planes_busy[i]) continue;
      hipEvent_t e = c->st.planes_ev[i];
      if (!e) {
        if (int rc = c->st.derive_fence[i].make(c, hipEventDisableTiming)) return rc;
        HIPCHK(c, hipEventRecord(c->st.derive_fence[i], busy[i]));
        planes_fenced(c, busy[i], e = c->st.derive_fence[i]);
      }
      for (int j = 0; j < n_derive_streams; j++) HIPCHK(c, hipStreamWaitEvent(c->st.derive_streams[j], e, 0));
    }
  }
  size_t k = 0;
  long long t_done = 0;                 // slices that are not tile aligned share a tile: it belongs to the earlier chunk
  for (const SubSlice &sl : plan) {
    const long long t0 = std::max(t_done, (long long)(sl.first / 64)), t1 = (long long)((sl.first + sl.n + 63) / 64);
    if (t0 >= t1) continue;
    t_done = t1;
    hipStream_t ds = c->st.derive_streams[k % (size_t)n_derive_streams];
    int rc = for_owned_tiles(c, t0, t1, [&](long long, long long lt, long long nt) -> int { return derive_rows(c, c->db, lt * 64, (int)(nt * 64), ds, true); });
    if (rc) return rc;
    if (k == c->st.derive_chunks.size()) {   // (a chunk's event is made behind its launch: the first launch waits for nothing it does not need)
      c->st.derive_chunks.emplace_back();
      if (int rc = c->st.derive_chunks.back().done.make(c, hipEventDisableTiming)) { c->st.derive_chunks.pop_back(); return rc; }
    }
    c->st.derive_chunks[k].t0 = t0; c->st.derive_chunks[k].t1 = t1;
    HIPCHK(c, hipEventRecord(c->st.derive_chunks[k].done, ds));
    k++;
  }
  c->st.derive_pending = k;
  return 0;
}

// Two streams and a ring of NBUF counter buffers: the scan needs no state, so it runs up to NBUF-1 slices ahead of the replay.
// snapshot >= 0: the first pool's snapshot is given (query shards: the maximum over all ranks); only valid for a single pool.
static int run_subslices(uvaia_gpu_ctx *c, const std::vector<SubSlice> &subs, int64_t ordinal_of_db0, int snapshot)
{
  const size_t ns = subs.size();
  size_t issued = 0;
  {   // a launch of fewer waves than ~2 rounds of the chip's 8 192 wave slots leaves it half empty at start and end: let such
      // launches of consecutive slices overlap (they write different buffers)
    const int nqt = (c->act_q1 + 15) / 16 - c->act_q0 / 16;
    size_t longest = 0;
    for (const SubSlice &sl : subs) longest = std::max(longest, sl.n);
    const size_t waves = ns ? (size_t)nqt * ((longest + 63) / 64) : 0;
    // (a single query tile: the scan is bound by HBM, launches next to each other only slow each other down)
    // (round 4: with 63 query tiles three overlapping scans of 25 000 references ran at 1.4 ms each instead of 0.63 -- their blocks
    // interleave and every XCD's L2 serves three times the reference pairs; only launches of less than two rounds overlap)
    // (and with the scan-side extras over the column-compressed scan -- tuning.replay_extras = 2, 33-128 queries -- the replays on their own
    // compute units are the chain: scans in order, each done as early as can be; three at a time 5.25 ms of scans + replays per million
    // references at 64 queries, one after the other 4.40.  Without the extras the three streams stand: 7.98 against 8.22 ms per step.)
    c->st.scan_nstreams = (waves && waves < 16000 && nqt >= 4 && !c->use_ext) ? 3 : 1;
    if (c->st.scan_nstreams_forced) c->st.scan_nstreams = c->st.scan_nstreams_forced;
  }
  for (size_t i = 0; i < ns; i++) {
    const bool serial_ = c->serial;
    while (issued < ns && issued < i + (serial_ ? 1 : NBUF)) {          // keep the scan stream fed
      int rc = uvaia_gpu_slice_scan(c, subs[issued].first, subs[issued].n, (int)(issued % NBUF));
      if (rc) return rc;
      issued++;
      if (serial_) (void)sync_scan_streams(c);
    }
    int take = subs[i].pool_start ? 1 : 0;
    if (take && snapshot >= 0) { HIPCHK(c, hipMemcpyAsync(c->state.d_snap, &snapshot, sizeof(int), hipMemcpyHostToDevice, c->st.stream)); HIPCHK(c, hipStreamSynchronize(c->st.stream)); take = 0; }
    int rc = uvaia_gpu_slice_replay(c, (int)(i % NBUF), ordinal_of_db0 + (long long)subs[i].first, take);
    if (rc) return rc;
    if (serial_) hipStreamSynchronize(c->st.stream);
  }
  return 0;
}

int uvaia_gpu_search_resident(uvaia_gpu_ctx *c, size_t pool, int64_t ordinal0, uint8_t *entered)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: use uvaia_gpu_shard_scan / uvaia_gpu_shard_replay (or a group)");
  if (pool < 1 || pool > c->max_pool) return fail(c, UVAIA_GPU_EINVAL, "pool must be in [1, max_pool=%zu]", c->max_pool);
  if (!c->db_n) return 0;
  // the flags of this search only: cleared here unless uvaia_gpu_reset has just done it (no replay since: launch_replay withdraws the mark)
  if (c->state.entered_clean < ((c->db_n + 63) / 64) * 64) HIPCHK(c, hipMemsetAsync(c->state.d_entered, 0, ((c->db_n + 63) / 64) * 64, c->st.stream));
  c->state.entered_clean = 0;
  if (!c->fullscan) {
    int rc = run_subslices(c, plan_subslices(c, 0, c->db_n, pool), ordinal0, -1);
    if (rc) return rc;
  } else
  for (size_t a = 0; a < c->db_n; a += pool) {
    const size_t b = std::min(c->db_n, a + pool);
    const long long tf = (long long)(a / 64);
    const int n_tiles = (int)((b + 63) / 64 - a / 64);
    const int rb = (int)(a - (size_t)tf * 64), re = (int)(b - (size_t)tf * 64);
    int rc = run_batch(c, c->db, tf, n_tiles, rb, re, ordinal0 + (long long)a);
    if (rc) return rc;
  }
  if (entered) {
    HIPCHK(c, hipMemcpyAsync(entered, c->state.d_entered, c->db_n, hipMemcpyDeviceToHost, c->st.stream));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    return collect_events(c);
  }
  return 0;
}

int uvaia_gpu_search_resident_pool(uvaia_gpu_ctx *c, size_t first, size_t n, int64_t ordinal0, int snapshot)
{ // one batch ("pool") [first, first + n) of the resident database; entered flags accumulate (uvaia_gpu_entered_flags)
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->fullscan) return fail(c, UVAIA_GPU_ESTATE, "per-pool search needs the default scan");
  if (n < 1 || n > c->max_pool || first + n > c->db_n) return fail(c, UVAIA_GPU_EINVAL, "pool [%zu,+%zu) outside the database or above max_pool=%zu", first, n, c->max_pool);
  return run_subslices(c, plan_subslices(c, first, n, n), ordinal0 - (int64_t)first, snapshot);
}

int uvaia_gpu_sync(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = sync_derive_streams(c)) return rc;
  c->st.derive_pending = 0;
  if (int rc = sync_scan_streams(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (c->st.rep_stream) HIPCHK(c, hipStreamSynchronize(c->st.rep_stream));
  planes_idle(c, true, true);
  return collect_events(c);
}

int uvaia_gpu_last_batch_scores(uvaia_gpu_ctx *c, int *out, int n_ref)
{
  if (!c || !out) return UVAIA_GPU_EINVAL;
  if (n_ref != c->last.n || !c->last.store) return fail(c, UVAIA_GPU_ESTATE, "last batch held %d references, not %d", c->last.n, n_ref);
  const int *nonn = c->last.store->nonn + c->last.tile_first * 64;
  DevBuf<int> d_out;
  const size_t bytes = (size_t)n_ref * c->nq * 6 * sizeof(int);
  if (!c->fullscan) {   // the production path keeps two counters per pair: recount the batch with the four-counter kernel
    int rc = ensure_cnt4(c, (size_t)c->nq_pad * c->last.ppad); if (rc) return rc;
    const bool prof = c->stats.profile; c->stats.profile = false;
    rc = launch_scan(c, *c->last.store, c->last.tile_first, c->last.n_tiles, c->tab.d_qp, c->nq, c->state.d_cnt, c->last.ppad, 0.0);
    c->stats.profile = prof;
    if (rc) return rc;
  }
  if (int rc = d_out.reserve(c, bytes / sizeof(int))) return rc;
  dim3 grid((n_ref + 255) / 256, c->nq);
  if (c->acgt) hipLaunchKernelGGL((batch_scores_kernel<true>), grid, dim3(256), 0, c->st.stream, c->state.d_cnt, c->last.ppad, c->last.rt, nonn, c->last.rbegin, n_ref, c->nq, d_out);
  else         hipLaunchKernelGGL((batch_scores_kernel<false>), grid, dim3(256), 0, c->st.stream, c->state.d_cnt, c->last.ppad, c->last.rt, nonn, c->last.rbegin, n_ref, c->nq, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->st.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
  if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "batch_scores: %s", hipGetErrorString(e));
  return 0;
}

int uvaia_gpu_scan_stats(uvaia_gpu_ctx *c, double *ms, long long *launches, double *bytes, int reset)
{
  if (!c) return UVAIA_GPU_EINVAL;
  int rc = collect_events(c); if (rc) return rc;
  if (ms) *ms = c->stats.scan_ms;
  if (launches) *launches = c->stats.scan_launches;
  if (bytes) *bytes = c->stats.scan_bytes;
  if (reset) { c->stats.scan_ms = 0; c->stats.scan_bytes = 0; c->stats.scan_launches = 0; }
  return 0;
}

int uvaia_gpu_replay_stats(uvaia_gpu_ctx *c, unsigned long long out[3], int reset)
{
  if (!c || !out) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  unsigned long long h[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpy(h, c->stats.d_stats, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
  if (reset) HIPCHK(c, hipMemset(c->stats.d_stats, 0, sizeof h));
  return 0;
}

int uvaia_gpu_replay_timing(uvaia_gpu_ctx *c, unsigned long long out[12], int reset)
{ // diagnostics of an engine built with -DREPLAY_TIMING (zeros otherwise): wall-clock ticks (100 MHz) summed over the replay waves --
  // waiting for staged counters, requesting them, inside opened tiles, of that inside admissions, late fetches, their number, whole waves
  if (!c || !out) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  HIPCHK(c, hipMemcpy(out, c->stats.d_stats + 4, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(c, hipMemset(c->stats.d_stats + 4, 0, 12 * sizeof(unsigned long long)));
  return 0;
}

int uvaia_gpu_replay_tiles_opened(uvaia_gpu_ctx *c, unsigned long long *out, int reset)
{ // (query, tile of 64 references) pairs whose counters the replay of the packed-plane scan looked at since the last reset
  if (!c || !out) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  unsigned long long h3 = 0;
  HIPCHK(c, hipMemcpy(&h3, c->stats.d_stats + 3, sizeof h3, hipMemcpyDeviceToHost));
  *out = h3;
  if (reset) HIPCHK(c, hipMemset(c->stats.d_stats + 3, 0, sizeof h3));
  return 0;
}

// ---- ring mode (multi-GPU, DESIGN.md "Multi-GPU"): the database is dealt block-cyclically, every rank scans its slice
// of a stripe concurrently, and the small per-query state travels rank to rank so that each query still sees the
// references in stream order.  state blob = snapshot, n[q], T[q], heap[q][k+1][8]  (all int32).
size_t uvaia_gpu_state_range_bytes(const uvaia_gpu_ctx *c, int q0, int q1)
{
  if (!c || q0 < 0 || q1 > c->nq || q1 < q0) return 0;
  const size_t nqr = (size_t)(q1 - q0);
  return sizeof(int) * (4 + 2 * nqr + nqr * (c->k + 1) * HEAP_ENTRY);
}
size_t uvaia_gpu_state_bytes(const uvaia_gpu_ctx *c) { return c ? uvaia_gpu_state_range_bytes(c, 0, c->nq) : 0; }

int uvaia_gpu_state_export_range(uvaia_gpu_ctx *c, void *dst, int q0, int q1)
{ // dst: device (or host) memory of uvaia_gpu_state_range_bytes(); ordered on the replay stream, then waited for
  if (!c || !dst || q0 < 0 || q1 > c->nq || q1 < q0) return UVAIA_GPU_EINVAL;
  int *d = (int *)dst;
  const size_t nqr = (size_t)(q1 - q0), he = (size_t)(c->k + 1) * HEAP_ENTRY;
  HIPCHK(c, hipMemcpyAsync(d, c->state.d_snap, sizeof(int), hipMemcpyDefault, c->st.stream));
  if (nqr) {
    HIPCHK(c, hipMemcpyAsync(d + 4, c->state.d_n + q0, nqr * sizeof(int), hipMemcpyDefault, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(d + 4 + nqr, c->state.d_T + q0, nqr * sizeof(int), hipMemcpyDefault, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(d + 4 + 2 * nqr, c->state.d_heap + (size_t)q0 * he, nqr * he * sizeof(int), hipMemcpyDefault, c->st.stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

int uvaia_gpu_state_import_range(uvaia_gpu_ctx *c, const void *src, int q0, int q1)
{
  if (!c || !src || q0 < 0 || q1 > c->nq || q1 < q0) return UVAIA_GPU_EINVAL;
  const int *d = (const int *)src;
  const size_t nqr = (size_t)(q1 - q0), he = (size_t)(c->k + 1) * HEAP_ENTRY;
  HIPCHK(c, hipMemcpyAsync(c->state.d_snap, d, sizeof(int), hipMemcpyDefault, c->st.stream));
  if (nqr) {
    HIPCHK(c, hipMemcpyAsync(c->state.d_n + q0, d + 4, nqr * sizeof(int), hipMemcpyDefault, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(c->state.d_T + q0, d + 4 + nqr, nqr * sizeof(int), hipMemcpyDefault, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(c->state.d_heap + (size_t)q0 * he, d + 4 + 2 * nqr, nqr * he * sizeof(int), hipMemcpyDefault, c->st.stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));     // src may be reused or freed once this returns
  return 0;
}

int uvaia_gpu_state_export(uvaia_gpu_ctx *c, void *dst) { return c ? uvaia_gpu_state_export_range(c, dst, 0, c->nq) : UVAIA_GPU_EINVAL; }
int uvaia_gpu_state_import(uvaia_gpu_ctx *c, const void *src) { return c ? uvaia_gpu_state_import_range(c, src, 0, c->nq) : UVAIA_GPU_EINVAL; }

// counts of database references [first, first+n) into counter buffer `buf` (0 .. NBUF-1), asynchronously on a scan stream
int uvaia_gpu_slice_scan(uvaia_gpu_ctx *c, size_t first, size_t n, int buf)
{
  if (!c || buf < 0 || buf >= NBUF) return UVAIA_GPU_EINVAL;
  if (c->fullscan) return fail(c, UVAIA_GPU_ESTATE, "ring mode needs the two-counter scan");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: use uvaia_gpu_shard_scan / uvaia_gpu_shard_replay");
  if (first + n > c->db_n) return fail(c, UVAIA_GPU_EINVAL, "slice [%zu,+%zu) outside the database", first, n);
  // a slice is at most a pool when the batch snapshot can matter (n_idx_c > 0); otherwise pools have no effect and slices are free
  if (n > c->max_pool && c->n_idx_c > 0) return fail(c, UVAIA_GPU_EINVAL, "slice of %zu references above max_pool %zu", n, c->max_pool);
  SliceBuf &b = c->slice[buf];
  const size_t ppad_ = ((first + n + 63) / 64 - first / 64) * 64;
  // the scans write whole query tiles up to the last active one: super-tiles of 64 queries (scan3_kernel), tiles of 16 otherwise
  const size_t qtile = c->scan_variant == 2 ? 64 : 16;
  const size_t rows = std::min<size_t>((size_t)c->nq_pad, ((size_t)c->act_q1 + qtile - 1) / qtile * qtile);
  if (int rc = slice_reserve(c, b, rows * ppad_, ppad_)) return rc;
  hipStream_t ss = c->st.scan_streams[c->st.scan_nstreams > 1 ? (c->st.scan_rr++ % c->st.scan_nstreams) : 0];
  if (b.replay_recorded) HIPCHK(c, hipStreamWaitEvent(ss, b.replay_done, 0));   // the buffer's previous reader
  for (size_t k = 0; k < c->st.derive_pending; k++) {                                          // planes being rebuilt (uvaia_gpu_db_rederive)
    const auto &d = c->st.derive_chunks[k];
    if (d.t0 < (long long)((first + n + 63) / 64) && d.t1 > (long long)(first / 64)) HIPCHK(c, hipStreamWaitEvent(ss, d.done, 0));
  }
  b.tf = (long long)(first / 64);
  b.tiles = n ? (int)((first + n + 63) / 64 - first / 64) : 0;
  b.rb = (int)(first - (size_t)b.tf * 64); b.re = b.rb + (int)n;
  b.scanned = true; b.cons_done = false;
  const double bytes = (double)n * (double)c->W4 * 16.0 * c->P + (double)c->nq * (double)c->W4 * 16.0 * c->P;
  int rc = launch_scan2(c, c->db, b.tf, b.tiles, b.cnt, b.tiles * 64, bytes, ss, b.tmin, b.rb, b.re, b.rt, c->use_ext ? b.ext : nullptr, b.rtp, b.tb8);
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(b.scan_done, ss));
  planes_fenced(c, ss, b.scan_done);
  return 0;
}

// gate + heaps of queries [q0,q1) over the slice scanned into `buf`, from the state currently held (imported or local).
// take_snapshot != 0: this call opens a batch for the whole query set, so the batch snapshot (cq->max_incompatible,
// src/nearest.c:290-291) is taken from the state of ALL queries now held; otherwise the imported snapshot is used.
int uvaia_gpu_slice_replay_range(uvaia_gpu_ctx *c, int buf, int64_t ordinal0, int q0, int q1, int take_snapshot)
{
  if (!c || buf < 0 || buf >= NBUF) return UVAIA_GPU_EINVAL;
  SliceBuf &b = c->slice[buf];
  if (!b.scanned) return fail(c, UVAIA_GPU_ESTATE, "slice_replay without slice_scan");
  if (q0 < 0 || q1 > c->nq || q1 < q0) return fail(c, UVAIA_GPU_EINVAL, "bad query range [%d,%d)", q0, q1);
  if (take_snapshot) { hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(256), 0, c->st.stream, c->state.d_T + c->act_q0, c->act_q1 - c->act_q0, c->state.d_snap); b.cons_done = false; }
  if (b.re <= b.rb || q1 == q0) return 0;
  HIPCHK(c, hipStreamWaitEvent(c->st.stream, b.scan_done, 0));
  const int ppad = b.tiles * 64;
  // (packed-plane scan, default mode: the scan left every counter of every pair -- the replay without a round trip per admission)
  const uint32_t *ext = c->use_ext ? b.ext : nullptr;
  // (the replay's own compute units: the kernel runs on the masked stream, spliced into c->st.stream's order by two events)
  hipStream_t rs = (c->st.rep_stream && ext) ? c->st.rep_stream : c->st.stream;
  if (rs != c->st.stream) { HIPCHK(c, hipEventRecord(c->st.rep_ev[0], c->st.stream)); HIPCHK(c, hipStreamWaitEvent(rs, c->st.rep_ev[0], 0)); }
  // Candidates of a tile whose on-demand counters are requested ahead.  The bookkeeping of the request slots costs more than the
  // latency it hides (measured on one box: config[1] 3.69 / 3.54 / 3.60 ms per step with 3 / 2 / 1, 4 queries x 1 M references
  // 4.37 / 4.03 / 3.89; with 6 or 8 over 7 ms): two for large query sets, one -- request, then use -- for a handful of queries.
  const int pf = (q1 - q0) <= 64 ? 1 : 2;
  int rc = launch_replay(c, {rs, q0, q1, b.cnt, ext, ppad, b.rt, b.rtp, b.tmin, b.tb8,
                             c->db.planes, b.tf, c->db.nonn + b.tf * 64, c->db.amb + b.tf * 64 * AMB_ROW, c->state.d_entered + b.tf * 64, b.rb, b.re, (long long)ordinal0,
                             (c->scan_variant == 2 && c->shard.world == 1) ? c->tab.d_qpl : nullptr, c->db.poly, c->tab.NR4, c->tab.d_qrare, pf});
  if (rc) return rc;
  if (rs != c->st.stream) { HIPCHK(c, hipEventRecord(c->st.rep_ev[1], rs)); HIPCHK(c, hipStreamWaitEvent(c->st.stream, c->st.rep_ev[1], 0)); }
  HIPCHK(c, hipEventRecord(b.replay_done, c->st.stream));
  planes_fenced(c, c->st.stream, b.replay_done);
  b.replay_recorded = true;
  c->last = {&c->db, b.tf, b.tiles, b.re - b.rb, b.rb, ppad, b.rt};
  return 0;
}

int uvaia_gpu_slice_buffers(void) { return NBUF; }

int uvaia_gpu_slice_replay(uvaia_gpu_ctx *c, int buf, int64_t ordinal0, int stripe_start)
{ return c ? uvaia_gpu_slice_replay_range(c, buf, ordinal0, c->act_q0, c->act_q1, stripe_start) : UVAIA_GPU_EINVAL; }

int uvaia_gpu_set_active_queries(uvaia_gpu_ctx *c, int q0, int q1)
{
  if (!c) return UVAIA_GPU_EINVAL;
  // (with reference shards the range only selects whose tolerances uvaia_gpu_max_tolerance looks at -- every scan covers all queries --
  // and may start anywhere; a range that is scanned starts at a super-tile of 64 queries)
  if (q0 < 0 || q1 > c->nq || q1 <= q0 || ((q0 % 64) && c->shard.world == 1))
    return fail(c, UVAIA_GPU_EINVAL, "active queries [%d,%d): need 0 <= q0 < q1 <= %d and q0 a multiple of 64", q0, q1, c->nq);
  if ((c->fullscan || c->scan_variant != 2) && c->shard.world == 1) { if (q0 != 0 || q1 != c->nq) return fail(c, UVAIA_GPU_ESTATE, "query shards need the default scan"); }
  c->act_q0 = q0; c->act_q1 = q1;
  return 0;
}

int uvaia_gpu_max_tolerance(uvaia_gpu_ctx *c, int *out)
{ // max over the active queries of max_incompatible: a rank's contribution to the batch snapshot (src/nearest.c:290-291)
  if (!c || !out) return UVAIA_GPU_EINVAL;
  DevBuf<int> d_tmp;
  if (int rc = d_tmp.reserve(c, 1)) return rc;
  hipLaunchKernelGGL(snapshot_kernel, dim3(1), dim3(256), 0, c->st.stream, c->state.d_T + c->act_q0, c->act_q1 - c->act_q0, d_tmp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_tmp, sizeof(int), hipMemcpyDeviceToHost, c->st.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
  if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "max_tolerance: %s", hipGetErrorString(e));
  return 0;
}

int uvaia_gpu_entered_flags(uvaia_gpu_ctx *c, uint8_t *out, int clear)
{ // "entered any heap" flags of the resident database accumulated by slice replays (and by search_resident)
  if (!c) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (out && c->db_n) HIPCHK(c, hipMemcpy(out, c->state.d_entered, c->db_n, hipMemcpyDeviceToHost));
  if (clear && c->db_n) HIPCHK(c, hipMemset(c->state.d_entered, 0, ((c->db_n + 63) / 64) * 64));
  return 0;
}


}  // extern "C"
