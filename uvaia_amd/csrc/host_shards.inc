// host_shards.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): reference shards: per-context shard calls, ordering against caller streams, the group of contexts driven by one host thread.

extern "C" {

// ---- reference shards (several GPUs; DESIGN.md "Multi-GPU").  Every context holds the packed planes of ALL references (what the
// replay's on-demand counters read; query-independent, loaded once) but derives and scans only its share: the stream is dealt in
// pieces of piece_refs references (whole tiles), piece p belongs to rank p % world.  A rank scans a piece against ALL queries into
// caller-owned buffers, the caller moves the rows of each query shard to the rank that replays those queries (RCCL all-to-all
// between processes, peer copies inside one: uvaia_gpu_group_*), and every rank replays its queries over the pieces in stream order.
int uvaia_gpu_db_set_shard(uvaia_gpu_ctx *c, int rank, int world, size_t piece_refs)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (world < 1 || rank < 0 || rank >= world) return fail(c, UVAIA_GPU_EINVAL, "rank %d of %d", rank, world);
  if (world > 64) return fail(c, UVAIA_GPU_EINVAL, "reference shards: at most 64 ranks, all on one node (a rank reads the others' packed planes in place: peer or hipIpc mappings); got %d", world);
  if (world > 1 && (piece_refs < 64 || piece_refs % 64 || piece_refs > c->max_pool)) return fail(c, UVAIA_GPU_EINVAL, "a piece holds a whole number of tiles of 64 references, at most max_pool = %zu (got %zu)", c->max_pool, piece_refs);
  if (c->db.planes || c->db_n) return fail(c, UVAIA_GPU_ESTATE, "the reference shard is set before the database is reserved");
  if (world > 1 && c->fullscan) return fail(c, UVAIA_GPU_ESTATE, "reference shards need the two-counter scans (alignments up to 49 000 columns)");
  c->shard.rank = rank; c->shard.world = world; c->shard.pt = world > 1 ? (long long)(piece_refs / 64) : 0;
  return 0;
}

int uvaia_gpu_shard_rows(const uvaia_gpu_ctx *c) { return c ? c->nq_pad : 0; }

// Pair counters of the references [first, first + n) (inside one piece of this context's shard) against ALL queries:
//   cnt  [uvaia_gpu_shard_rows()][tiles * 64] int2,  tmin [uvaia_gpu_shard_rows()][tiles] int2,  tiles = the tiles the range touches;
// a reference sits in column (its position - 64 * (first / 64)).  Asynchronous; uvaia_gpu_scan_wait() waits for the scans issued so far.
size_t uvaia_gpu_shard_aux_bytes(const uvaia_gpu_ctx *c, size_t n_tiles)
{ // per reference of a piece, what its replay needs besides the pair counters: valid sites (4 bytes) and, with constant-and-complete
  // query columns, the untruncated consensus pre-score (16 bytes)
  return c ? n_tiles * 64 * (sizeof(int) + (c->n_idx_c > 0 ? sizeof(int4) : 0)) : 0;
}

int uvaia_gpu_shard_scan(uvaia_gpu_ctx *c, size_t first, size_t n, void *cnt, void *tmin, void *aux)
{
  if (!c || !cnt || !tmin || !aux) return c ? fail(c, UVAIA_GPU_EINVAL, "NULL buffer") : UVAIA_GPU_EINVAL;
  if (c->fullscan) return fail(c, UVAIA_GPU_ESTATE, "reference shards need the two-counter scans");
  if (n < 1 || first + n > c->db_n) return fail(c, UVAIA_GPU_EINVAL, "range [%zu,+%zu) outside the database", first, n);
  const long long tf = (long long)(first / 64);
  const int n_tiles = (int)((first + n + 63) / 64 - first / 64);
  if ((size_t)n_tiles * 64 > c->pool_pad) return fail(c, UVAIA_GPU_EINVAL, "range of %zu references above max_pool %zu", n, c->max_pool);
  if (c->shard.world > 1 && (!owns_tile(c, tf) || tf / c->shard.pt != (tf + n_tiles - 1) / c->shard.pt))
    return fail(c, UVAIA_GPU_ESTATE, "references [%zu,+%zu) are not inside one piece of this context's reference shard", first, n);
  const long long ltf = dtile_of(c, tf);            // the context's own number of the piece's first tile
  hipStream_t ss = c->st.scan_streams[0];
  for (size_t k = 0; k < c->st.derive_pending; k++) {
    const auto &d = c->st.derive_chunks[k];
    if (d.t0 < tf + n_tiles && d.t1 > tf) HIPCHK(c, hipStreamWaitEvent(ss, d.done, 0));
  }
  const int rb = (int)(first - (size_t)tf * 64);
  const double bytes = (double)n * (double)c->W4 * 16.0 * c->P + (double)c->nq * (double)c->W4 * 16.0 * c->P;
  int rc = launch_scan2(c, c->db, ltf, n_tiles, (uint32_t *)cnt, n_tiles * 64, bytes, ss, (int2 *)tmin, rb, rb + (int)n, c->slice[0].rt);
  if (rc) return rc;
  // what travels with the counters: the references' valid sites and their consensus pre-score
  const size_t cols = (size_t)n_tiles * 64;
  HIPCHK(c, hipMemcpyAsync(aux, c->db.nonn + ltf * 64, cols * sizeof(int), hipMemcpyDeviceToDevice, ss));
  if (c->n_idx_c > 0) HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char *>(aux) + cols * sizeof(int), c->slice[0].rt, cols * sizeof(int4), hipMemcpyDeviceToDevice, ss));
  return 0;
}

int uvaia_gpu_scan_wait(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  return sync_scan_streams(c);
}

// waits for the replays issued so far (their counter buffers may then be overwritten); scans keep running
int uvaia_gpu_replay_wait(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

// ---- ordering against a stream the caller owns (the stream its collectives run on) by events, without involving the host: what lets
// the reference-shard driver queue scan -> exchange -> replay of stripe after stripe asynchronously (uvaia_amd/refshard.py).
// A mark = the scans (or replays) issued so far, remembered under a slot number; a caller stream can be made to wait for a mark, and
// the engine's later scans (or replays) for what a caller stream holds now.
int uvaia_gpu_mark(uvaia_gpu_ctx *c, int what, int slot)
{
  if (!c || slot < 0 || slot >= 8 || (what != UVAIA_GPU_SCANS && what != UVAIA_GPU_REPLAYS)) return c ? fail(c, UVAIA_GPU_EINVAL, "mark: what = scans or replays, slot 0..7") : UVAIA_GPU_EINVAL;
  for (int i = 0; i < 3; i++) {
    Event &e = c->st.mark_ev[slot][i];
    hipStream_t st = what == UVAIA_GPU_SCANS ? c->st.scan_streams[i] : (i == 0 ? c->st.stream : nullptr);
    c->st.mark_set[slot][i] = false;
    if (!st) continue;
    if (int rc = e.make(c, hipEventDisableTiming)) return rc;
    HIPCHK(c, hipEventRecord(e, st));
    c->st.mark_set[slot][i] = true;
  }
  return 0;
}
int uvaia_gpu_stream_wait_mark(uvaia_gpu_ctx *c, void *stream, int slot)
{
  if (!c || slot < 0 || slot >= 8) return c ? fail(c, UVAIA_GPU_EINVAL, "slot 0..7") : UVAIA_GPU_EINVAL;
  for (int i = 0; i < 3; i++) if (c->st.mark_set[slot][i]) HIPCHK(c, hipStreamWaitEvent((hipStream_t)stream, c->st.mark_ev[slot][i], 0));
  return 0;
}
int uvaia_gpu_wait_stream(uvaia_gpu_ctx *c, int what, void *stream)
{
  if (!c || (what != UVAIA_GPU_SCANS && what != UVAIA_GPU_REPLAYS)) return c ? fail(c, UVAIA_GPU_EINVAL, "wait_stream: what = scans or replays") : UVAIA_GPU_EINVAL;
  Event &e = c->st.order_ev[c->st.order_rr++ % 16];
  if (int rc = e.make(c, hipEventDisableTiming)) return rc;
  HIPCHK(c, hipEventRecord(e, (hipStream_t)stream));
  if (what == UVAIA_GPU_REPLAYS) HIPCHK(c, hipStreamWaitEvent(c->st.stream, e, 0));
  else for (int i = 0; i < 3; i++) if (c->st.scan_streams[i]) HIPCHK(c, hipStreamWaitEvent(c->st.scan_streams[i], e, 0));
  return 0;
}

// cq->max_incompatible of the batch that starts now (src/nearest.c:290-291), given by the caller: the maximum over the ranks of
// uvaia_gpu_max_tolerance().  Only matters when the query set has constant-and-complete columns.
int uvaia_gpu_set_snapshot(uvaia_gpu_ctx *c, int snapshot)
{
  if (!c) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipMemcpyAsync(c->state.d_snap, &snapshot, sizeof(int), hipMemcpyHostToDevice, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

// Where the packed planes and side rows of rank `rank`'s pieces can be read from by this context's kernels: device pointers valid in
// this process (a member of a group hands over its own; between processes uvaia_gpu_shard_ipc_handles / _open).  The replay reads
// them for the few pairs that reach the exact comparison.
int uvaia_gpu_shard_set_peer(uvaia_gpu_ctx *c, int rank, const void *planes, const void *side_rows)
{
  if (!c || rank < 0 || rank >= 64 || rank >= std::max(1, c->shard.world)) return c ? fail(c, UVAIA_GPU_EINVAL, "rank %d", rank) : UVAIA_GPU_EINVAL;
  c->shard.peer_db[rank] = (const uint4 *)planes; c->shard.peer_amb[rank] = (const int *)side_rows;
  return 0;
}
const void *uvaia_gpu_shard_planes(const uvaia_gpu_ctx *c) { return c ? c->db.planes : nullptr; }
const void *uvaia_gpu_shard_side_rows(const uvaia_gpu_ctx *c) { return c ? c->db.amb : nullptr; }
int uvaia_gpu_shard_ipc_handle_bytes(void) { return 2 * (int)sizeof(hipIpcMemHandle_t); }
int uvaia_gpu_shard_ipc_handles(uvaia_gpu_ctx *c, void *out)
{ // inter-process handles of this context's packed planes and side rows (after uvaia_gpu_db_reserve)
  if (!c || !out) return UVAIA_GPU_EINVAL;
  if (!c->db.planes || !c->db.amb) return fail(c, UVAIA_GPU_ESTATE, "reserve the database first");
  hipIpcMemHandle_t h[2];
  HIPCHK(c, hipIpcGetMemHandle(&h[0], c->db.planes));
  HIPCHK(c, hipIpcGetMemHandle(&h[1], c->db.amb));
  memcpy(out, h, sizeof h);
  return 0;
}
int uvaia_gpu_shard_ipc_open(uvaia_gpu_ctx *c, int rank, const void *handles)
{ // maps another process's arrays (its uvaia_gpu_shard_ipc_handles) as the source of rank `rank`'s pieces
  if (!c || !handles || rank < 0 || rank >= 64 || rank >= c->shard.world || rank == c->shard.rank) return c ? fail(c, UVAIA_GPU_EINVAL, "rank %d", rank) : UVAIA_GPU_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  hipIpcMemHandle_t h[2];
  memcpy(h, handles, sizeof h);
  for (int i = 0; i < 2; i++) if (c->shard.ipc_opened[rank][i]) { hipIpcCloseMemHandle(c->shard.ipc_opened[rank][i]); c->shard.ipc_opened[rank][i] = nullptr; }
  HIPCHK(c, hipIpcOpenMemHandle(&c->shard.ipc_opened[rank][0], h[0], hipIpcMemLazyEnablePeerAccess));
  HIPCHK(c, hipIpcOpenMemHandle(&c->shard.ipc_opened[rank][1], h[1], hipIpcMemLazyEnablePeerAccess));
  c->shard.peer_db[rank] = (const uint4 *)c->shard.ipc_opened[rank][0]; c->shard.peer_amb[rank] = (const int *)c->shard.ipc_opened[rank][1];
  return 0;
}

int uvaia_gpu_shard_ipc_close(uvaia_gpu_ctx *c)
{ // unmaps what uvaia_gpu_shard_ipc_open mapped: before the ranks that own the arrays free them (every rank closes, then a barrier, then the contexts go)
  if (!c) return UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  for (int r = 0; r < 64; r++) {
    bool any = false;
    for (int i = 0; i < 2; i++) if (c->shard.ipc_opened[r][i]) { hipIpcCloseMemHandle(c->shard.ipc_opened[r][i]); c->shard.ipc_opened[r][i] = nullptr; any = true; }
    if (any) { c->shard.peer_db[r] = nullptr; c->shard.peer_amb[r] = nullptr; }
  }
  return 0;
}

// Gate + heaps of queries [q0, q1) over references [first, first + n) -- a piece scanned by rank `owner` -- from counters laid out as
// uvaia_gpu_shard_scan writes them but holding the rows of queries q0 .. q1-1 only (row 0 = query q0), and the piece's `aux` block.
// Asynchronous on the replay stream; the buffers must stay valid and complete until uvaia_gpu_sync().
int uvaia_gpu_shard_replay(uvaia_gpu_ctx *c, const void *cnt, const void *tmin, const void *aux, int owner, size_t first, size_t n, int64_t ordinal0, int q0, int q1)
{
  if (!c || !cnt || !tmin || !aux) return c ? fail(c, UVAIA_GPU_EINVAL, "NULL buffer") : UVAIA_GPU_EINVAL;
  if (c->fullscan) return fail(c, UVAIA_GPU_ESTATE, "reference shards need the two-counter scans");
  if (q0 < 0 || q1 > c->nq || q1 < q0) return fail(c, UVAIA_GPU_EINVAL, "bad query range [%d,%d)", q0, q1);
  if (first + n > c->db_n) return fail(c, UVAIA_GPU_EINVAL, "range [%zu,+%zu) outside the database", first, n);
  if (n < 1 || q1 == q0) return 0;
  const long long tf = (long long)(first / 64);
  const int n_tiles = (int)((first + n + 63) / 64 - first / 64), ppad = n_tiles * 64;
  if ((size_t)ppad > c->pool_pad) return fail(c, UVAIA_GPU_EINVAL, "range of %zu references above max_pool %zu", n, c->max_pool);
  if (owner < 0 || owner >= std::max(1, c->shard.world) || (c->shard.world > 1 && (int)((tf / c->shard.pt) % c->shard.world) != owner))
    return fail(c, UVAIA_GPU_EINVAL, "references [%zu,+%zu) are not a piece of rank %d", first, n, owner);
  if (!c->shard.peer_db[owner] || (!c->acgt && !c->shard.peer_amb[owner])) return fail(c, UVAIA_GPU_ESTATE, "the arrays of rank %d are not known to this context (uvaia_gpu_shard_set_peer / uvaia_gpu_shard_ipc_open)", owner);
  const int rb = (int)(first - (size_t)tf * 64), re = rb + (int)n;
  const long long ltf = dtile_of(c, tf);            // the piece's first tile in its owner's numbering
  // the kernel indexes rows by query number: shift the bases so that row q0 is the buffer's first row
  const uint32_t *cntp = (const uint32_t *)cnt - (ptrdiff_t)q0 * ppad;
  const int2 *tminp = (const int2 *)tmin - (ptrdiff_t)q0 * (ppad / 64);
  const int *nonn = (const int *)aux;
  const int4 *rt = c->n_idx_c > 0 ? (const int4 *)(reinterpret_cast<const char *>(aux) + (size_t)ppad * sizeof(int)) : c->state.d_rt;
  const int *amb = c->shard.peer_amb[owner] ? c->shard.peer_amb[owner] + ltf * 64 * AMB_ROW : nullptr;
  // the owner's packed planes and side rows; no derived planes of another rank: the on-demand counters come from the packed ones
  // (--acgt: dist_unique of the pairs that reach a heap is counted from them too, the scan's per-pair count stays on the scanning rank)
  return launch_replay(c, {c->st.stream, q0, q1, cntp, nullptr, ppad, rt, nullptr, tminp, nullptr,
                           c->shard.peer_db[owner], ltf, nonn, amb, c->state.d_entered + tf * 64, rb, re, (long long)ordinal0,
                           nullptr, nullptr, 0, nullptr, 3});
}

// ---- a group of contexts in ONE process (the C command line's --devices): the reference-shard protocol above with peer copies as
// the exchange.  Replaces the batch loop of src/nearest.c:245-330 for several GPUs.  One host thread drives all devices: every
// step is an asynchronous launch or copy, ordered by events across the devices' streams.
// One host thread per member device: a stripe of a sharded search is a few dozen asynchronous launches and copies PER MEMBER (scan,
// three peer copies per owner, a replay per piece, the events between them); issued by one thread for eight devices they take longer
// than the devices need to run them.  The workers live as long as the group; `run` hands every worker the same function with its
// member number and returns when all have come back (two such rounds per stripe: the scans, whose events the second round waits for,
// then fetches and replays).
struct GroupWorkers {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv, cv_done;
  std::function<int(int)> job;
  unsigned gen = 0;
  int pending = 0;
  bool stop = false;
  std::vector<int> rc;
  void start(int n, const std::vector<int> &devices)
  {
    rc.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) th.emplace_back([this, i, dev = devices[(size_t)i]]() {
      (void)hipSetDevice(dev);
      unsigned seen = 0;
      for (;;) {
        std::function<int(int)> f;
        { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&]() { return stop || gen != seen; }); if (stop) return; seen = gen; f = job; }
        const int r = f(i);
        { std::lock_guard<std::mutex> lk(m); rc[(size_t)i] = r; if (--pending == 0) cv_done.notify_all(); }
      }
    });
  }
  int run(const std::function<int(int)> &f)            // first non-zero return code of the members, in member order
  {
    if (th.empty()) return 0;
    { std::lock_guard<std::mutex> lk(m); job = f; pending = (int)th.size(); gen++; }
    cv.notify_all();
    { std::unique_lock<std::mutex> lk(m); cv_done.wait(lk, [&]() { return pending == 0; }); }
    for (int r : rc) if (r) return r;
    return 0;
  }
  void shutdown()
  {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv.notify_all();
    for (auto &t : th) if (t.joinable()) t.join();
    th.clear();
  }
};

struct uvaia_gpu_group {
  int n = 0, nq = 0, rows = 0, cons = 0;
  GroupWorkers workers;                         // one thread per member (n > 1)
  std::vector<std::string> merr;                // a worker's error message, per member
  size_t piece = 0, aux_piece = 0;
  std::vector<uvaia_gpu_ctx *> ctx;
  std::vector<int> q0, q1;                      // query shard of each member (multiples of 16)
  struct Member {
    uint32_t *send_cnt[2] = {}, *recv_cnt[2] = {};
    int2 *send_tmin[2] = {}, *recv_tmin[2] = {};
    char *send_aux[2] = {}, *recv_aux[2] = {};       // per reference of a piece: valid sites, consensus pre-score (uvaia_gpu_shard_aux_bytes)
    hipStream_t copy = nullptr;
    hipEvent_t scanned[2] = {}, fetched[2] = {}, replayed[2] = {};    // scan into send[b] done; this member's copies out of everyone's send[b] done; replays from recv[b] done
    bool fetched_rec[2] = {}, replayed_rec[2] = {};
  };
  std::vector<Member> m;
  std::string err;
};

static int gfail(uvaia_gpu_group *g, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (g) g->err = buf; else g_open_error = buf;
  return code;
}
#define GCHK(g, call) HIP_TRY(call, return gfail((g), UVAIA_GPU_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__))
#define GCTX(g, i, call) do { int rc_ = (call); if (rc_) return gfail((g), rc_, "device %d: %s", (g)->ctx[(size_t)(i)]->device, uvaia_gpu_last_error((g)->ctx[(size_t)(i)])); } while (0)

const char *uvaia_gpu_group_last_error(const uvaia_gpu_group *g) { return g ? g->err.c_str() : g_open_error.c_str(); }
int uvaia_gpu_group_size(const uvaia_gpu_group *g) { return g ? g->n : 0; }
uvaia_gpu_ctx *uvaia_gpu_group_member(uvaia_gpu_group *g, int i) { return (g && i >= 0 && i < g->n) ? g->ctx[(size_t)i] : nullptr; }

void uvaia_gpu_group_close(uvaia_gpu_group *g)
{
  if (!g) return;
  g->workers.shutdown();
  // Members read each other's arrays in place (packed planes and side rows through peer pointers, the send buffers through the copy
  // streams): everything in flight on EVERY device ends before anything of ANY member is freed (errors ignored: this is the way out)
  for (int i = 0; i < (int)g->ctx.size(); i++) {
    if (!g->ctx[(size_t)i]) continue;
    hipSetDevice(g->ctx[(size_t)i]->device);
    if (i < (int)g->m.size() && g->m[(size_t)i].copy) hipStreamSynchronize(g->m[(size_t)i].copy);
    uvaia_gpu_sync(g->ctx[(size_t)i]);
  }
  for (int i = 0; i < (int)g->ctx.size(); i++) {
    if (!g->ctx[(size_t)i]) continue;
    hipSetDevice(g->ctx[(size_t)i]->device);
    if (i < (int)g->m.size()) {
      auto &mm = g->m[(size_t)i];
      if (mm.copy) hipStreamDestroy(mm.copy);
      for (int b = 0; b < 2; b++) {
        void *p[] = {mm.send_cnt[b], mm.send_tmin[b], mm.recv_cnt[b], mm.recv_tmin[b], mm.send_aux[b], mm.recv_aux[b]};
        for (void *x : p) if (x) hipFree(x);
        hipEvent_t ev[] = {mm.scanned[b], mm.fetched[b], mm.replayed[b]};
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
      }
    }
    uvaia_gpu_close(g->ctx[(size_t)i]);
  }
  delete g;
}

// devices[i]: HIP device of member i (a device may be listed more than once: several contexts on one GPU).  piece_refs: references per
// piece of the shard map (multiple of 64, at most max_pool); 0 = max_pool rounded down to whole tiles, at most 8 192.
int uvaia_gpu_group_open(uvaia_gpu_group **out, const uvaia_gpu_query *q, int heap_size, const int *devices, int n_devices, size_t max_pool, size_t piece_refs)
{
  if (!out) return gfail(nullptr, UVAIA_GPU_EINVAL, "group is NULL");
  *out = nullptr;
  if (!devices || n_devices < 1 || n_devices > 64) return gfail(nullptr, UVAIA_GPU_EINVAL, "1 to 64 devices");
  if (max_pool < 64 && n_devices > 1) return gfail(nullptr, UVAIA_GPU_EINVAL, "several devices need max_pool >= 64");
  uvaia_gpu_group *g = new uvaia_gpu_group();
  g->n = n_devices;
  g->piece = n_devices == 1 ? 0 : (piece_refs ? piece_refs : std::min<size_t>(8192, max_pool / 64 * 64));
  if (g->n > 1 && (g->piece < 64 || g->piece % 64 || g->piece > max_pool)) { delete g; return gfail(nullptr, UVAIA_GPU_EINVAL, "piece of %zu references: need a multiple of 64 up to max_pool", piece_refs); }
  g->ctx.assign((size_t)g->n, nullptr);
  for (int i = 0; i < g->n; i++) {
    int rc = uvaia_gpu_open(&g->ctx[(size_t)i], q, heap_size, devices[i], max_pool);
    if (rc) { uvaia_gpu_group_close(g); return rc; }                      // message already in the open error
    rc = uvaia_gpu_db_set_shard(g->ctx[(size_t)i], i, g->n, g->piece);
    if (rc) { gfail(nullptr, rc, "%s", uvaia_gpu_last_error(g->ctx[(size_t)i])); uvaia_gpu_group_close(g); return rc; }
  }
  g->nq = q->n_query; g->rows = g->ctx[0]->nq_pad; g->cons = q->n_idx_c > 0;
  {   // contiguous query shards, whole query tiles
    int per = (g->nq + g->n - 1) / g->n; per = (per + 15) / 16 * 16;
    for (int i = 0; i < g->n; i++) { const int a = std::min(g->nq, i * per); g->q0.push_back(a); g->q1.push_back(std::min(g->nq, a + per)); }
  }
  g->m.resize((size_t)g->n);
  if (g->n > 1) {
    const size_t pcols = g->piece + 64;                      // a range that starts inside a tile touches one tile more
    g->aux_piece = uvaia_gpu_shard_aux_bytes(g->ctx[0], pcols / 64);
    for (int i = 0; i < g->n; i++) {
      auto &mm = g->m[(size_t)i];
      const size_t myrows = (size_t)std::max(1, g->q1[(size_t)i] - g->q0[(size_t)i]);
      hipError_t e = hipSetDevice(g->ctx[(size_t)i]->device);
      if (e == hipSuccess) e = hipStreamCreateWithFlags(&mm.copy, hipStreamNonBlocking);
      for (int b = 0; b < 2 && e == hipSuccess; b++) {
        e = hipMalloc(&mm.send_cnt[b], (size_t)g->rows * pcols * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&mm.send_tmin[b], (size_t)g->rows * (pcols / 64) * sizeof(int2));
        if (e == hipSuccess) e = hipMalloc(&mm.recv_cnt[b], (size_t)g->n * myrows * pcols * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&mm.recv_tmin[b], (size_t)g->n * myrows * (pcols / 64) * sizeof(int2));
        if (e == hipSuccess) e = hipMalloc(&mm.send_aux[b], g->aux_piece);
        if (e == hipSuccess) e = hipMalloc(&mm.recv_aux[b], (size_t)g->n * g->aux_piece);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mm.scanned[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mm.fetched[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&mm.replayed[b], hipEventDisableTiming);
      }
      if (e != hipSuccess) { const int code = gfail(nullptr, e == hipErrorOutOfMemory ? UVAIA_GPU_ENOMEM : UVAIA_GPU_EHIP, "group buffers on device %d: %s", devices[i], hipGetErrorString(e)); uvaia_gpu_group_close(g); return code; }
      for (int j = 0; j < g->n; j++) if (devices[j] != devices[i]) { int can = 0; if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) { hipError_t pe = hipDeviceEnablePeerAccess(devices[j], 0); if (pe == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError(); } }
    }
  }
  if (g->n > 1) {
    g->merr.assign((size_t)g->n, std::string());
    g->workers.start(g->n, std::vector<int>(devices, devices + n_devices));
  }
  *out = g;
  return 0;
}

int uvaia_gpu_group_query_shard(const uvaia_gpu_group *g, int i, int *q0, int *q1)
{ if (!g || i < 0 || i >= g->n || !q0 || !q1) return UVAIA_GPU_EINVAL; *q0 = g->q0[(size_t)i]; *q1 = g->q1[(size_t)i]; return 0; }

#define EACH_MEMBER(g, expr) do { for (int i_ = 0; i_ < (g)->n; i_++) { GCHK(g, hipSetDevice((g)->ctx[(size_t)i_]->device)); uvaia_gpu_ctx *cx = (g)->ctx[(size_t)i_]; GCTX(g, i_, (expr)); } } while (0)
int uvaia_gpu_group_db_reserve(uvaia_gpu_group *g, size_t cap)
{ // every member keeps the packed planes, side rows and derived planes of its own pieces, and learns where the others keep theirs
  // (one process: the members' device pointers serve, peer access was enabled by the open)
  if (!g) return UVAIA_GPU_EINVAL;
  EACH_MEMBER(g, uvaia_gpu_db_reserve(cx, cap));
  if (g->n > 1) for (int i = 0; i < g->n; i++) for (int j = 0; j < g->n; j++)
    GCTX(g, i, uvaia_gpu_shard_set_peer(g->ctx[(size_t)i], j, uvaia_gpu_shard_planes(g->ctx[(size_t)j]), uvaia_gpu_shard_side_rows(g->ctx[(size_t)j])));
  return 0;
}
int uvaia_gpu_group_db_clear(uvaia_gpu_group *g) { if (!g) return UVAIA_GPU_EINVAL; EACH_MEMBER(g, uvaia_gpu_db_clear(cx)); return 0; }
int uvaia_gpu_group_reset(uvaia_gpu_group *g) { if (!g) return UVAIA_GPU_EINVAL; EACH_MEMBER(g, uvaia_gpu_reset(cx)); return 0; }
int uvaia_gpu_group_sync(uvaia_gpu_group *g)
{
  if (!g) return UVAIA_GPU_EINVAL;
  for (int i = 0; i < g->n; i++) { GCHK(g, hipSetDevice(g->ctx[(size_t)i]->device)); if (g->m[(size_t)i].copy) GCHK(g, hipStreamSynchronize(g->m[(size_t)i].copy)); GCTX(g, i, uvaia_gpu_sync(g->ctx[(size_t)i])); }
  return 0;
}
// every member is handed the whole stream and keeps the references of its own pieces (packed planes, side rows, derived planes)
// (an append to an empty database that was never reserved reserves for it: through the group, so that the members learn each other's arrays)
static int group_room_for(uvaia_gpu_group *g, int n_ref)
{
  if (n_ref > 0 && g->ctx[0]->db_n == 0 && (size_t)n_ref > g->ctx[0]->db_cap) return uvaia_gpu_group_db_reserve(g, (size_t)n_ref);
  return 0;
}
int uvaia_gpu_group_db_append(uvaia_gpu_group *g, const char *const *seq, const int *non_n, int n_ref)
{ if (!g) return UVAIA_GPU_EINVAL; { int rc = group_room_for(g, n_ref); if (rc) return rc; } EACH_MEMBER(g, uvaia_gpu_db_append(cx, seq, non_n, n_ref)); return 0; }
int uvaia_gpu_group_db_append_packed(uvaia_gpu_group *g, const void *planes, const int *non_n, const int *side_rows, int n_ref)
{ if (!g) return UVAIA_GPU_EINVAL; { int rc = group_room_for(g, n_ref); if (rc) return rc; } EACH_MEMBER(g, uvaia_gpu_db_append_packed(cx, planes, non_n, side_rows, n_ref)); return 0; }
int uvaia_gpu_group_db_rederive(uvaia_gpu_group *g) { if (!g) return UVAIA_GPU_EINVAL; EACH_MEMBER(g, uvaia_gpu_db_rederive(cx)); return 0; }
size_t uvaia_gpu_group_db_size(const uvaia_gpu_group *g) { return g ? uvaia_gpu_db_size(g->ctx[0]) : 0; }
#undef EACH_MEMBER

// The whole while-loop of src/nearest.c:249-330 over the resident database in batches of `pool` references, sharded: per batch
// the snapshot of the tolerances is the maximum over ALL members' heaps (src/nearest.c:290-291; only taken when the query set has
// constant-and-complete columns, otherwise batches have no effect); the pieces of the shard map inside the batch are scanned by
// their owners, `n` pieces (one per member) at a time, the rows of every query shard are copied to the member that replays them,
// and each member replays its queries over the pieces in stream order.  Asynchronous unless entered != NULL.
int uvaia_gpu_group_search_resident(uvaia_gpu_group *g, size_t pool, int64_t ordinal0, uint8_t *entered)
{
  if (!g) return UVAIA_GPU_EINVAL;
  const size_t total = uvaia_gpu_db_size(g->ctx[0]);
  if (g->n == 1) {
    GCHK(g, hipSetDevice(g->ctx[0]->device));
    GCTX(g, 0, uvaia_gpu_search_resident(g->ctx[0], pool, ordinal0, entered));
    return 0;
  }
  if (pool < 1) return gfail(g, UVAIA_GPU_EINVAL, "pool must be positive");
  for (int i = 0; i < g->n; i++) {
    if (uvaia_gpu_db_size(g->ctx[(size_t)i]) != total) return gfail(g, UVAIA_GPU_ESTATE, "members hold different databases");
    GCHK(g, hipSetDevice(g->ctx[(size_t)i]->device));
    GCHK(g, hipMemsetAsync(g->ctx[(size_t)i]->state.d_entered, 0, ((total + 63) / 64) * 64, g->ctx[(size_t)i]->st.stream));
  }
  if (!total) return 0;
  if (!g->cons) pool = total;                          // batches act through the snapshot only (see plan_subslices)
  struct Piece { size_t first, n; int owner; };
  unsigned stripe_no = 0;
  // inside a worker: the member's message goes to its own slot, the code comes back through GroupWorkers::run
#define WCHK(i, call) HIP_TRY(call, { char b_[384]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); g->merr[(size_t)(i)] = b_; return UVAIA_GPU_EHIP; })
#define WCTX(i, call) do { const int rc_ = (call); if (rc_) { g->merr[(size_t)(i)] = std::string("device ") + std::to_string(g->ctx[(size_t)(i)]->device) + ": " + uvaia_gpu_last_error(g->ctx[(size_t)(i)]); return rc_; } } while (0)
  auto run_members = [&](const std::function<int(int)> &f) -> int {
    const int rc = g->workers.run(f);
    if (rc) for (int i = 0; i < g->n; i++) if (!g->merr[(size_t)i].empty()) { gfail(g, rc, "%s", g->merr[(size_t)i].c_str()); g->merr[(size_t)i].clear(); break; }
    return rc;
  };
  for (size_t a = 0; a < total; a += pool) {
    const size_t b = std::min(total, a + pool);
    if (g->cons) {   // the batch snapshot: needs every member's tolerances as the previous batch left them
      std::vector<int> tol((size_t)g->n, -0x7fffffff);
      int rc = run_members([&](int i) -> int {
        uvaia_gpu_ctx *cx = g->ctx[(size_t)i];
        if (g->q1[(size_t)i] <= g->q0[(size_t)i]) return 0;
        WCHK(i, hipSetDevice(cx->device));
        const int a0 = cx->act_q0, a1 = cx->act_q1;
        cx->act_q0 = g->q0[(size_t)i]; cx->act_q1 = g->q1[(size_t)i];
        int v = 0; const int got = uvaia_gpu_max_tolerance(cx, &v);
        cx->act_q0 = a0; cx->act_q1 = a1;
        WCTX(i, got);
        tol[(size_t)i] = v;
        return 0;
      });
      if (rc) return rc;
      const int snap = *std::max_element(tol.begin(), tol.end());
      rc = run_members([&](int i) -> int { WCHK(i, hipSetDevice(g->ctx[(size_t)i]->device)); WCTX(i, uvaia_gpu_set_snapshot(g->ctx[(size_t)i], snap)); return 0; });
      if (rc) return rc;
    }
    std::vector<Piece> pieces;                          // the parts of the shard map's pieces inside [a, b), in stream order
    for (size_t x = a; x < b;) { const size_t pe = std::min(b, (x / g->piece + 1) * g->piece); pieces.push_back({x, pe - x, (int)((x / g->piece) % (size_t)g->n)}); x = pe; }
    for (size_t s0 = 0; s0 < pieces.size(); s0 += (size_t)g->n, stripe_no++) {
      const size_t s1 = std::min(pieces.size(), s0 + (size_t)g->n);
      const int bsel = (int)(stripe_no & 1u);
      // 1. scans, each by its owner's thread (consecutive pieces have distinct owners); a send buffer is reused once everyone has fetched from it
      //    (the `fetched` events of two stripes ago were recorded before this round began: the rounds are separated by the workers' hand-back)
      int rc = run_members([&](int i) -> int {
        for (size_t k = s0; k < s1; k++) {
          const Piece &pc = pieces[k];
          if (pc.owner != i) continue;
          uvaia_gpu_ctx *cx = g->ctx[(size_t)i]; auto &mo = g->m[(size_t)i];
          WCHK(i, hipSetDevice(cx->device));
          for (int d = 0; d < g->n; d++) if (g->m[(size_t)d].fetched_rec[bsel]) WCHK(i, hipStreamWaitEvent(cx->st.scan_streams[0], g->m[(size_t)d].fetched[bsel], 0));
          WCTX(i, uvaia_gpu_shard_scan(cx, pc.first, pc.n, mo.send_cnt[bsel], mo.send_tmin[bsel], mo.send_aux[bsel]));
          WCHK(i, hipEventRecord(mo.scanned[bsel], cx->st.scan_streams[0]));
        }
        return 0;
      });
      if (rc) return rc;
      // 2. every member fetches the rows of its queries from every owner, 3. and replays them in stream order
      rc = run_members([&](int d) -> int {
        auto &md = g->m[(size_t)d]; uvaia_gpu_ctx *cd = g->ctx[(size_t)d];
        const size_t myrows = (size_t)(g->q1[(size_t)d] - g->q0[(size_t)d]);
        WCHK(d, hipSetDevice(cd->device));
        if (md.replayed_rec[bsel]) WCHK(d, hipStreamWaitEvent(md.copy, md.replayed[bsel], 0));      // the receive buffer's previous readers
        for (size_t k = s0; k < s1 && myrows; k++) {
          const Piece &pc = pieces[k]; auto &mo = g->m[(size_t)pc.owner];
          const size_t tiles = (pc.first + pc.n + 63) / 64 - pc.first / 64, ppad = tiles * 64, slot = k - s0;
          WCHK(d, hipStreamWaitEvent(md.copy, mo.scanned[bsel], 0));
          WCHK(d, hipMemcpyPeerAsync(md.recv_cnt[bsel] + slot * myrows * (g->piece + 64), cd->device, mo.send_cnt[bsel] + (size_t)g->q0[(size_t)d] * ppad, g->ctx[(size_t)pc.owner]->device,
                                     myrows * ppad * sizeof(uint32_t), md.copy));
          WCHK(d, hipMemcpyPeerAsync(md.recv_tmin[bsel] + slot * myrows * ((g->piece + 64) / 64), cd->device, mo.send_tmin[bsel] + (size_t)g->q0[(size_t)d] * tiles, g->ctx[(size_t)pc.owner]->device,
                                     myrows * tiles * sizeof(int2), md.copy));
          WCHK(d, hipMemcpyPeerAsync(md.recv_aux[bsel] + slot * g->aux_piece, cd->device, mo.send_aux[bsel], g->ctx[(size_t)pc.owner]->device, uvaia_gpu_shard_aux_bytes(cd, tiles), md.copy));
        }
        WCHK(d, hipEventRecord(md.fetched[bsel], md.copy)); md.fetched_rec[bsel] = true;
        WCHK(d, hipStreamWaitEvent(cd->st.stream, md.fetched[bsel], 0));
        for (size_t k = s0; k < s1 && myrows; k++) {
          const Piece &pc = pieces[k]; const size_t slot = k - s0;
          WCTX(d, uvaia_gpu_shard_replay(cd, md.recv_cnt[bsel] + slot * myrows * (g->piece + 64), md.recv_tmin[bsel] + slot * myrows * ((g->piece + 64) / 64),
                                         md.recv_aux[bsel] + slot * g->aux_piece, pc.owner, pc.first, pc.n, ordinal0 + (int64_t)pc.first, g->q0[(size_t)d], g->q1[(size_t)d]));
        }
        WCHK(d, hipEventRecord(md.replayed[bsel], cd->st.stream)); md.replayed_rec[bsel] = true;
        return 0;
      });
      if (rc) return rc;
    }
  }
#undef WCHK
#undef WCTX
  if (entered) {   // a reference is dumped if it entered the heap of ANY query (src/nearest.c:303-306): OR over the members
    std::vector<uint8_t> part(total);
    memset(entered, 0, total);
    for (int i = 0; i < g->n; i++) {
      GCHK(g, hipSetDevice(g->ctx[(size_t)i]->device));
      if (g->m[(size_t)i].copy) GCHK(g, hipStreamSynchronize(g->m[(size_t)i].copy));
      GCTX(g, i, uvaia_gpu_sync(g->ctx[(size_t)i]));
      GCTX(g, i, uvaia_gpu_entered_flags(g->ctx[(size_t)i], part.data(), 0));
      for (size_t x = 0; x < total; x++) entered[x] |= part[x];
    }
  }
  return 0;
}

// one batch of the reference loop, sequences from host memory (uvaia_gpu_push for the group): every member packs the batch, the
// scan of its pieces is shared out as above
int uvaia_gpu_group_push(uvaia_gpu_group *g, const char *const *seq, const int *non_n, int n_ref, int64_t ordinal0, uint8_t *entered)
{
  if (!g) return UVAIA_GPU_EINVAL;
  if (n_ref < 0 || (n_ref > 0 && !seq)) return gfail(g, UVAIA_GPU_EINVAL, "bad batch");
  if (n_ref == 0) return 0;
  if (g->n == 1) { GCHK(g, hipSetDevice(g->ctx[0]->device)); GCTX(g, 0, uvaia_gpu_push(g->ctx[0], seq, non_n, n_ref, ordinal0, entered)); return 0; }
  int rc = uvaia_gpu_group_sync(g); if (rc) return rc;
  rc = uvaia_gpu_group_db_clear(g); if (rc) return rc;
  rc = uvaia_gpu_group_db_append(g, seq, non_n, n_ref); if (rc) return rc;
  std::vector<uint8_t> ent((size_t)n_ref);
  rc = uvaia_gpu_group_search_resident(g, (size_t)n_ref, ordinal0, entered ? entered : ent.data());
  return rc;
}

// heaps of all queries, each from the member that replays it (arrays as uvaia_gpu_drain)
int uvaia_gpu_group_drain(uvaia_gpu_group *g, int *n_items, int *max_incompatible, int *scores, int64_t *ordinals)
{
  if (!g || !n_items || !scores || !ordinals) return UVAIA_GPU_EINVAL;
  if (g->n == 1) { GCHK(g, hipSetDevice(g->ctx[0]->device)); GCTX(g, 0, uvaia_gpu_drain(g->ctx[0], n_items, max_incompatible, scores, ordinals)); return 0; }
  const size_t slots = (size_t)uvaia_gpu_heap_slots(g->ctx[0]) + 1;
  std::vector<int> n((size_t)g->nq), T((size_t)g->nq), sc((size_t)g->nq * slots * 6);
  std::vector<int64_t> od((size_t)g->nq * slots);
  for (int i = 0; i < g->n; i++) {
    GCHK(g, hipSetDevice(g->ctx[(size_t)i]->device));
    if (g->m[(size_t)i].copy) GCHK(g, hipStreamSynchronize(g->m[(size_t)i].copy));
    GCTX(g, i, uvaia_gpu_drain(g->ctx[(size_t)i], n.data(), T.data(), sc.data(), od.data()));
    for (int q = g->q0[(size_t)i]; q < g->q1[(size_t)i]; q++) {
      n_items[q] = n[(size_t)q];
      if (max_incompatible) max_incompatible[q] = T[(size_t)q];
      memcpy(scores + (size_t)q * slots * 6, sc.data() + (size_t)q * slots * 6, slots * 6 * sizeof(int));
      memcpy(ordinals + (size_t)q * slots, od.data() + (size_t)q * slots, slots * sizeof(int64_t));
    }
  }
  return 0;
}


}  // extern "C"
