// host_open.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): context life cycle: open (query planes, column classes, item streams), close, reset, the small getters.

extern "C" {

const char *uvaia_gpu_last_error(const uvaia_gpu_ctx *ctx) { return ctx ? ctx->err.c_str() : g_open_error.c_str(); }

void uvaia_gpu_close(uvaia_gpu_ctx *c)
{
  if (!c) return;
  // the streams that may still hold work are waited for; what was mapped from other processes is unmapped; everything else the context
  // holds goes with its members (host_ctx.inc)
  if (c->st.stream) hipStreamSynchronize(c->st.stream);
  if (c->win.copy_stream) hipStreamSynchronize(c->win.copy_stream);
  for (hipStream_t st : c->st.derive_streams) if (st) hipStreamSynchronize(st);
  if (c->st.rep_stream) hipStreamSynchronize(c->st.rep_stream);
  for (auto &rank : c->shard.ipc_opened) for (void *p : rank) if (p) hipIpcCloseMemHandle(p);
  delete c;
}

int uvaia_gpu_open(uvaia_gpu_ctx **out, const uvaia_gpu_query *q, int heap_size, int device, size_t max_pool)
{ return uvaia_gpu_open_tuned(out, q, heap_size, device, max_pool, nullptr); }

int uvaia_gpu_open_tuned(uvaia_gpu_ctx **out, const uvaia_gpu_query *q, int heap_size, int device, size_t max_pool, const uvaia_gpu_tuning *tune)
{
  uvaia_gpu_tuning tn;
  memset(&tn, 0, sizeof tn);
  if (tune) tn = *tune;
  if (tn.scan < 0 || tn.scan > UVAIA_GPU_SCAN_WIDE || tn.query_tables < 0 || tn.query_tables > 2 || (tn.scan_tiles_per_wave != 0 && tn.scan_tiles_per_wave != 1 && tn.scan_tiles_per_wave != 2 && tn.scan_tiles_per_wave != 4) ||
      (tn.scan_waves_per_block != 0 && tn.scan_waves_per_block != 4 && tn.scan_waves_per_block != 8) || (tn.subslice_refs != 0 && tn.subslice_refs < 64) ||
      (tn.derive_waves != 0 && tn.derive_waves != 4 && tn.derive_waves != 8 && tn.derive_waves != 16))
    return fail(nullptr, UVAIA_GPU_EINVAL, "bad tuning values");
  if (!out) return fail(nullptr, UVAIA_GPU_EINVAL, "ctx is NULL");
  *out = nullptr;
  if (!q || q->n_query < 1 || q->nchar < 1 || !q->seq || !q->consensus) return fail(nullptr, UVAIA_GPU_EINVAL, "empty or incomplete query set");
  if ((q->n_idx_c && !q->idx_c) || (q->n_idx_m && !q->idx_m) || (q->n_idx && !q->idx)) return fail(nullptr, UVAIA_GPU_EINVAL, "index arrays missing");
  if (max_pool < 1) return fail(nullptr, UVAIA_GPU_EINVAL, "max_pool must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, UVAIA_GPU_ENODEV, "no HIP device available: the MI355X engine has no CPU fallback");
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
  if (device >= ndev) return fail(nullptr, UVAIA_GPU_ENODEV, "device %d out of range (%d devices)", device, ndev);
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, UVAIA_GPU_ENODEV, "hipSetDevice(%d) failed", device);

  uvaia_gpu_ctx *c = new uvaia_gpu_ctx();
  c->device = device;
  c->nq = q->n_query; c->act_q0 = 0; c->act_q1 = q->n_query; c->nchar = q->nchar; c->acgt = q->acgt ? 1 : 0; c->trim = q->trim; c->n_idx_c = q->n_idx_c; c->n_idx_m = q->n_idx_m;
  c->P = c->acgt ? 3 : 4; c->NQ = c->acgt ? 4 : 6;
  c->W = (c->nchar + 31) / 32; c->W4 = (c->W + 3) / 4;
  c->k = heap_size < 2 ? 2 : heap_size;                      // src/min_heap.c:58
  c->qt = c->nq <= 8 ? 8 : 16;
  // Up to two query tiles: the column-compressed scan would move 25 KB per reference (building its planes) to read 1-8 KB; the
  // two-counter scan over the packed planes reads each reference once per query tile (15 KB) and needs nothing derived (DESIGN.md
  // 4.1; measured per 1 M references: 16 queries 5.3 ms against 8.8, 32 queries 8.2 against 9.8, 64 queries 12.6 against 8.9).
  c->scan_variant = tn.scan == UVAIA_GPU_SCAN_PACKED ? 0 : tn.scan == UVAIA_GPU_SCAN_COMPRESSED ? 2 : (c->nq <= 32 ? 0 : 2);
  c->fullscan = tn.scan == UVAIA_GPU_SCAN_WIDE;
  c->serial = tn.serial != 0;
  if (tn.scan_tiles_per_wave) c->scan_R = tn.scan_tiles_per_wave;
  if (tn.scan_waves_per_block) c->scan_NW = tn.scan_waves_per_block;
  if (c->scan_R == 4 && c->scan_NW != 8) { delete c; return fail(nullptr, UVAIA_GPU_EINVAL, "four reference tiles per wave go with eight waves per block"); }
  if (tn.subslice_refs) { c->subslice = tn.subslice_refs; c->subslice_forced = true; }
  if (tn.scan_streams >= 1 && tn.scan_streams <= 3) c->st.scan_nstreams_forced = tn.scan_streams;
  if (tn.scan_streams > 100 && tn.scan_streams < 200) c->first_slice_pct = tn.scan_streams == 199 ? 0 : tn.scan_streams - 100;
  c->derive_waves = tn.derive_waves;
  if (tn.ball_gather == 1 || tn.ball_gather == 2) c->ball.fused = tn.ball_gather == 2;
  if (tn.rederive_streams >= 1 && tn.rederive_streams <= 3) { c->st.derive_nstreams = tn.rederive_streams; c->st.derive_forced = true; }
  // the default scan keeps per-pair deficits in 16-bit halves (LDS counters): alignments of more than ~49 000 columns take the
  // four-counter scan instead (32-bit counts, same results, slower)
  if (c->nchar > 49000) c->fullscan = true;
  c->nq_pad = ((c->nq + 127) / 128) * 128;                   // multiple of every supported query tile and of the scan's super-tiles (64 or 128 queries)
  c->max_pool = max_pool; c->pool_pad = ((max_pool + 63) / 64) * 64 + 64;
  c->pitch = ((size_t)c->nchar + 63) / 64 * 64;
  if ((size_t)(c->k + 1) * HEAP_ENTRY * sizeof(int) + 128 > 160 * 1024) { delete c; return fail(nullptr, UVAIA_GPU_EINVAL, "nbest=%d does not fit the per-query LDS heap (max 5115)", heap_size); }

#define OPENCHK(call) HIP_TRY(call, { const int rc_ = fail(nullptr, code_, "%s failed: %s", #call, hipGetErrorString(e_)); uvaia_gpu_close(c); return rc_; })      /* while opening: the half-made context goes away */
#define OPENBUF(buf, n) do { if (const int rc_ = (buf).reserve(nullptr, (n))) { uvaia_gpu_close(c); return rc_; } } while (0)
  // packed-plane scan in default mode: the scan also leaves text - ACGT matches and partial - text matches of every pair (scan2_extras)
  // and the replay needs no memory round trip per admission (replay3_kernel)
  // (Over the column-compressed scan, 33-128 queries, two kernels after the scan can make the same arrays -- pair_extras_kernel,
  // tile_bounds_kernel -- but there it does not pay: the words the queries list cost 40 % of the packed bytes again, and replay2_kernel's
  // on-demand counters are no longer the step.  Per step of 1 M references, round 4: 64 queries 8.01 ms with, 7.98 without; 128 queries
  // 10.9 against 8.9; 40 queries 9.8 against 9.5.  Only on request: tuning replay_extras = 2.)
  c->use_ext = !c->fullscan && !c->acgt && tn.replay_extras != 1 && (c->scan_variant == 0 || (c->scan_variant == 2 && c->nq <= 128 && tn.replay_extras == 2));
  {  // the gate/replay stream outranks the scan stream: its few waves sit on the critical path of the state chain
    int prio_least = 0, prio_greatest = 0;
    OPENCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    // A handful of queries: the replay is a handful of waves bound by their own instruction stream (every counter they need is staged in
    // LDS ahead of them), and next to the waves of a scan that fills every SIMD they run three times slower than alone (measured, round 4:
    // the replay of 65 536 references x 4 queries 0.28 ms alone, 0.8 ms next to a scan).  So the replay gets compute units of its own --
    // one per XCD (the bits of a CU mask go round the XCDs), 32 SIMDs for at most 32 waves -- and the scans and the rebuild the other 248.
    bool split = false;
    // Every query's wave has to be resident at once (a second round of blocks would double the replay), one wave per SIMD where that fits:
    // the staging depth shrinks with the number of queries (LDS per block 84 KB / 52 KB / 35 KB at 32 / 16 / 8 tiles and nbest 100), and
    // the replay gets as many compute units as that takes -- 8 up to 32 queries, 16 up to 64, 32 up to 128.
    // (tuning: replay_cus = 1000 * tiles + units picks both, e.g. 16012)
    const int want_half = tn.replay_cus >= 1000 ? tn.replay_cus / 1000 : 0, want_cus = tn.replay_cus >= 1000 ? tn.replay_cus % 1000 : tn.replay_cus;
    c->replay_half = (want_half == 32 || want_half == 16 || want_half == 8) ? want_half : c->nq <= 8 ? 32 : c->nq <= 24 ? 16 : 8;
    int per_cu = (int)std::min<size_t>(4, (size_t)160 * 1024 / replay3_lds_bytes(c));
    while (c->use_ext && c->replay_half > 8 && per_cu * 8 < std::min(c->nq, 32)) { c->replay_half /= 2; per_cu = (int)std::min<size_t>(4, (size_t)160 * 1024 / replay3_lds_bytes(c)); }   // (a large nbest)
    // (a heap so large that even the shallowest staging does not fit next to it -- nbest above about 4 000 -- takes the on-demand replay)
    if (c->use_ext && replay3_lds_bytes(c) > (size_t)160 * 1024) c->use_ext = false;
    const int rep_cus = want_cus < 0 ? 0 : want_cus > 0 ? want_cus : (c->use_ext && per_cu > 0 ? std::max(8, ((c->nq + per_cu - 1) / per_cu + 7) / 8 * 8) : 0);
    hipDeviceProp_t prop;
    if (rep_cus > 0 && hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount >= 4 * rep_cus) {
      const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
      std::vector<uint32_t> m_rep((size_t)words, 0u), m_scan((size_t)words, 0u);
      for (int b = 0; b < ncu; b++) (b < rep_cus ? m_rep : m_scan)[(size_t)b >> 5] |= 1u << (b & 31);
      // (c->st.stream stays the stream everything of the replay is ordered on -- and the one packing, the radius search and the push path
      // run on, with the whole chip; a replay kernel of the resident search is put on rep_stream between two events: host_resident.inc)
      hipStream_t st[7] = {};
      bool ok = hipExtStreamCreateWithCUMask(&st[0], (uint32_t)words, m_rep.data()) == hipSuccess;
      for (int i = 1; i < 7 && ok; i++) ok = hipExtStreamCreateWithCUMask(&st[i], (uint32_t)words, m_scan.data()) == hipSuccess;
      if (ok) ok = hipEventCreateWithFlags(&c->st.rep_ev[0].e, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->st.rep_ev[1].e, hipEventDisableTiming) == hipSuccess;
      if (ok) {
        c->st.rep_stream.s = st[0];
        for (int i = 0; i < 3; i++) { c->st.scan_streams[i].s = st[1 + i]; c->st.derive_streams[i].s = st[4 + i]; }
        split = true; c->replay_cus = rep_cus;
      } else { (void)hipGetLastError(); for (int i = 0; i < 7; i++) if (st[i]) hipStreamDestroy(st[i]); }
    }
    OPENCHK(hipStreamCreateWithPriority(&c->st.stream.s, hipStreamNonBlocking, prio_greatest));
    if (!split) {
      for (int i = 0; i < 3; i++) OPENCHK(hipStreamCreateWithPriority(&c->st.scan_streams[i].s, hipStreamNonBlocking, prio_least));
      // between the scan (lowest) and the replay (highest): its blocks take the slots scan blocks free, ahead of the next scan blocks
      for (int i = 0; i < 3; i++) OPENCHK(hipStreamCreateWithPriority(&c->st.derive_streams[i].s, hipStreamNonBlocking, (prio_least + prio_greatest) / 2));
    }
    for (SliceBuf &b : c->slice) { OPENCHK(hipEventCreateWithFlags(&b.scan_done.e, hipEventDisableTiming)); OPENCHK(hipEventCreateWithFlags(&b.replay_done.e, hipEventDisableTiming)); }
  }
  uint8_t code_tab[256]; fill_code_table(code_tab);
  OPENCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_code), code_tab, 256));

  // ---- query planes (trimmed: sites outside [trim, nchar-trim) never count, src/fastaseq.c:744,750,763)
  const int lo = (int)std::min<size_t>(c->trim, (size_t)c->nchar), hi = std::max(lo, c->nchar - (int)c->trim);
  const size_t row_words = (size_t)c->W4 * 4 * c->NQ;
  std::vector<uint8_t> in_c(c->nchar, 0), in_m(c->nchar, 0), in_p(c->nchar, 0);
  for (int i = 0; i < q->n_idx_c; i++) if (q->idx_c[i] < (size_t)c->nchar) in_c[q->idx_c[i]] = 1;
  for (int i = 0; i < q->n_idx_m; i++) if (q->idx_m[i] < (size_t)c->nchar) in_m[q->idx_m[i]] = 1;
  for (int i = 0; i < q->n_idx; i++)   if (q->idx[i]   < (size_t)c->nchar) in_p[q->idx[i]] = 1;
  std::vector<uint32_t> cp(row_words, 0u), cpm(row_words, 0u);
  int bad = 0;
  for (int i = 0; i < c->nq; i++) if (!q->seq[i]) { uvaia_gpu_close(c); return fail(nullptr, UVAIA_GPU_EINVAL, "query %d is NULL", i); }
  if (pack_query_row(code_tab, q->consensus, c->nchar, 0, c->nchar, in_c.data(), nullptr, c->acgt, c->NQ, cp.data(), &bad) ||
      pack_query_row(code_tab, q->consensus, c->nchar, 0, c->nchar, in_m.data(), nullptr, c->acgt, c->NQ, cpm.data(), &bad)) {
    uvaia_gpu_close(c); return fail(nullptr, UVAIA_GPU_EALPHABET, "consensus holds byte 0x%02x outside the supported alphabet", bad);
  }
  {  // the queries restricted to query->idx are the query planes under the mask of those columns: kept as the mask (ensure_qpoly)
    std::vector<uint32_t> pmask((size_t)c->W4 * 4, 0u);
    for (int sidx = lo; sidx < hi; sidx++) if (in_p[(size_t)sidx]) pmask[(size_t)sidx >> 5] |= 1u << (sidx & 31);
    OPENBUF(c->tab.d_pmask, pmask.size()); OPENCHK(hipMemcpy(c->tab.d_pmask, pmask.data(), pmask.size() * 4, hipMemcpyHostToDevice));
    std::vector<int> cols;
    for (int sidx = lo; sidx < hi; sidx++) if (in_p[(size_t)sidx]) cols.push_back(sidx);
    c->ball.n_idx = (int)cols.size(); c->ball.NG4 = std::max(1, ((c->ball.n_idx + 31) / 32 + 3) / 4);
    c->ball.idx_cols = cols;
    cols.resize(cols.size() + 1, 0);
    OPENBUF(c->ball.d_idx_cols, cols.size()); OPENCHK(hipMemcpy(c->ball.d_idx_cols, cols.data(), cols.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  OPENBUF(c->d_stage, (size_t)2 * PACK_CHUNK * c->pitch);
  if (const int rc_ = c->h_stage.alloc(nullptr, (size_t)2 * PACK_CHUNK * c->pitch)) { uvaia_gpu_close(c); return rc_; }
  memset(c->h_stage, 'N', (size_t)2 * PACK_CHUNK * c->pitch);
  for (int i = 0; i < 2; i++) OPENCHK(hipEventCreateWithFlags(&c->stage_free[i].e, hipEventDisableTiming));
  // the query-side tables of the scans (query planes, column classes, rare columns, compressed planes, item streams): built on the
  // device from the raw rows (host_qprep.inc) or, on request, by host threads (host_qtables.inc); same bytes either way
  if (tn.query_tables == 1) { const int rc_ = build_query_tables_host(c, q, tn, code_tab, lo, hi, in_p); if (rc_) { uvaia_gpu_close(c); return rc_; } }
  else                      { const int rc_ = build_query_tables_device(c, q, tn, lo, hi);               if (rc_) { uvaia_gpu_close(c); return rc_; } }
  OPENBUF(c->tab.d_cp, cp.size()); OPENCHK(hipMemcpy(c->tab.d_cp, cp.data(), cp.size() * 4, hipMemcpyHostToDevice));
  OPENBUF(c->tab.d_cpm, cpm.size()); OPENCHK(hipMemcpy(c->tab.d_cpm, cpm.data(), cpm.size() * 4, hipMemcpyHostToDevice));

  // ---- state
  OPENBUF(c->state.d_heap, (size_t)c->nq * (c->k + 1) * HEAP_ENTRY);
  OPENBUF(c->state.d_n, (size_t)c->nq);
  OPENBUF(c->state.d_T, (size_t)c->nq);
  OPENBUF(c->state.d_snap, 1);
  OPENBUF(c->state.d_err, 1);
  OPENCHK(hipMemset(c->state.d_err, 0, sizeof(int)));
  // ---- batch buffers
  // (the buffers of a streamed batch -- packed tiles, their derived planes, side rows: 25 KB per reference of max_pool -- are allocated
  // by the first call that streams sequences in: ensure_batch_buffers)
  SliceBuf &b0 = c->slice[0];      // (the push path works in it: sized for a pool)
  if (!c->fullscan) OPENBUF(b0.cnt, (size_t)c->nq_pad * c->pool_pad);
  if (c->use_ext) {
    OPENBUF(b0.ext, (size_t)c->nq_pad * c->pool_pad);
    OPENBUF(b0.tb8, (size_t)c->nq_pad * (c->pool_pad / 64));
    OPENBUF(b0.rtp, c->pool_pad);
    OPENCHK(hipMemset(b0.rtp, 0, c->pool_pad * sizeof(uint32_t)));
    const size_t l3 = replay3_lds_bytes(c);
    // (every instantiation launch_replay can launch with more than the default dynamic LDS: here and below)
#define BIGLDS(K, N) OPENCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(N)))
    BIGLDS((replay3_kernel<true, 32>), l3); BIGLDS((replay3_kernel<false, 32>), l3); BIGLDS((replay3_kernel<true, 16>), l3);
    BIGLDS((replay3_kernel<false, 16>), l3); BIGLDS((replay3_kernel<true, 8>), l3); BIGLDS((replay3_kernel<false, 8>), l3);
  }
  OPENBUF(b0.tmin, (size_t)c->nq_pad * (c->pool_pad / 64));
  OPENBUF(b0.rt, c->pool_pad);
  OPENCHK(hipMemset(b0.rt, 0, c->pool_pad * sizeof(int4)));
  OPENBUF(c->stats.d_stats, 16);
  OPENCHK(hipMemset(c->stats.d_stats, 0, 16 * sizeof(unsigned long long)));
  OPENBUF(c->state.d_rt, c->pool_pad);
  OPENBUF(c->state.d_tr, c->pool_pad);
  OPENCHK(hipMemset(c->state.d_rt, 0, c->pool_pad * sizeof(int4)));      // stay zero when idx_c is empty (the pre-score is skipped)
  OPENCHK(hipMemset(c->state.d_tr, 0, c->pool_pad * sizeof(int4)));
  OPENBUF(c->state.d_entered, c->pool_pad);
  OPENCHK(hipMemset(c->state.d_entered, 0, c->pool_pad));
  const size_t lds = (size_t)(c->k + 1) * HEAP_ENTRY * sizeof(int) + 128;      // heap + the listed-words bitmap of replay2_kernel
  if (lds > 64 * 1024) {
    BIGLDS(replay_kernel<true>, lds); BIGLDS(replay_kernel<false>, lds);
#define BIGHEAP(PF_) BIGLDS((replay2_kernel<true, true, PF_>), lds); BIGLDS((replay2_kernel<true, false, PF_>), lds); BIGLDS((replay2_kernel<false, true, PF_>), lds); BIGLDS((replay2_kernel<false, false, PF_>), lds)
    BIGHEAP(1); BIGHEAP(2); BIGHEAP(3);
#undef BIGHEAP
  }
#undef BIGLDS
#undef OPENBUF
#undef OPENCHK
  int rc = uvaia_gpu_reset(c);
  if (rc) { g_open_error = c->err; uvaia_gpu_close(c); return rc; }
  *out = c;
  return UVAIA_GPU_OK;
}

int uvaia_gpu_export_query_table(uvaia_gpu_ctx *c, int which, void *out, size_t cap, size_t *n_bytes)
{
  if (!c || !n_bytes || which < 0 || which > 10) return UVAIA_GPU_EINVAL;
  if (which == 10) {
    const int v[11] = {c->tab.NP, c->tab.NR, c->tab.NP4, c->tab.NR4, c->tab.rare_max, c->scan_variant, c->tab.need_e_groups, c->tab.need_v_groups, c->tab.need_g_groups, c->tab.need_r_groups, c->replay_lq};
    *n_bytes = sizeof v;
    if (out && cap >= sizeof v) memcpy(out, v, sizeof v);
    return UVAIA_GPU_OK;
  }
  *n_bytes = c->tab.qtab[which].p ? c->tab.qtab[which].n : 0;
  if (out && *n_bytes && cap >= *n_bytes) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    HIPCHK(c, hipMemcpy(out, c->tab.qtab[which].p, *n_bytes, hipMemcpyDeviceToHost));
  }
  return UVAIA_GPU_OK;
}

int uvaia_gpu_reset(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  // One launch on `stream` and no wait for it: heaps, tolerances, item counts, the batch snapshot and the entered flags are only ever read
  // or written in `stream`'s order -- the replays and snapshots of every search path (push, resident, slices, reference shards and groups),
  // the state hand-over of the ring, uvaia_gpu_set_snapshot; the replay kernels of the masked replay stream run between two events of
  // `stream` (uvaia_gpu_slice_replay_range) -- and what the host reads (uvaia_gpu_drain, uvaia_gpu_entered_flags) waits for `stream` first.
  // The scans hold no such state: a step's first scan is issued while this kernel runs.
  const size_t heap16 = (size_t)c->nq * (c->k + 1) * HEAP_ENTRY * sizeof(int) / 16;
  const size_t ent = (c->state.d_entered && c->db_n) ? std::min(c->state.d_entered.cap / 64 * 64, ((c->db_n + 63) / 64) * 64) : 0;
  const size_t work = std::max(std::max(heap16, ent / 16), (size_t)c->nq);
  hipLaunchKernelGGL(reset_state_kernel, dim3((unsigned)std::min<size_t>(1024, (work + 255) / 256)), dim3(256), 0, c->st.stream,
                     reinterpret_cast<uint4 *>(c->state.d_heap.p), heap16, c->state.d_T, c->state.d_n, c->nq, c->nchar, c->state.d_snap, reinterpret_cast<uint4 *>(c->state.d_entered.p), ent / 16);
  HIPCHK(c, hipGetLastError());
  c->state.entered_clean = ent;
  return 0;
}

int uvaia_gpu_heap_slots(const uvaia_gpu_ctx *c) { return c ? c->k : 0; }
int uvaia_gpu_n_query(const uvaia_gpu_ctx *c) { return c ? c->nq : 0; }
size_t uvaia_gpu_packed_bytes_per_ref(const uvaia_gpu_ctx *c) { return c ? (size_t)c->W4 * 16 * c->P : 0; }
size_t uvaia_gpu_scan_bytes_per_ref(const uvaia_gpu_ctx *c)
{ // distinct bytes of a reference the default scan has to read at least once: the word groups of the two derived planes that
  // some query tile needs (groups where every query is clean are never loaded) + three planes of the gathered polymorphic columns
  if (!c) return 0;
  return (c->fullscan || c->scan_variant != 2) ? (size_t)c->W4 * 16 * c->P
                                                : (size_t)(c->tab.need_e_groups + c->tab.need_v_groups) * 16 + (size_t)c->tab.need_g_groups * 4 + (size_t)(c->tab.NP4 + c->tab.need_r_groups) * 16 * 3;
}

int uvaia_gpu_scan_variant(const uvaia_gpu_ctx *c)
{ // which pair scan this context runs: 2 column-compressed (scan3_kernel), 0 two counters over the packed planes (scan2_*_kernel;
  // default for at most 32 queries), -1 four counters (alignments above 49 000 columns)
  return !c ? -2 : c->fullscan ? -1 : c->scan_variant;
}

size_t uvaia_gpu_derived_bytes_per_ref(const uvaia_gpu_ctx *c)
{ // bytes per reference uvaia_gpu_db_rederive writes for the open query set (E, group counts, gathered columns, total)
  if (!c || c->fullscan || c->scan_variant != 2) return 0;
  return (size_t)c->W4 * 16 + (size_t)c->W4 * 4 + (size_t)(c->tab.NP4 + c->tab.NR4) * 48 + 4;   // E, grp, gathered planes, total; V is written once by the appends
}

int uvaia_gpu_set_query_tile(uvaia_gpu_ctx *c, int qt)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (qt == 0) qt = 16;
  if (qt != 8 && qt != 16 && qt != 32) return fail(c, UVAIA_GPU_EINVAL, "query tile must be 8, 16 or 32");
  c->qt = qt;
  return 0;
}


}  // extern "C"
