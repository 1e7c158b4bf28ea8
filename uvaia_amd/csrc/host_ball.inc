// host_ball.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the radius search of uvaiaball.

extern "C" {

// radius search over references [r_lo, r_hi) (relative to tile tile_first of `planes`, the packed tiles of a store: nothing else of it is
// read): stage 1 for all, the queries for the few
static int ball_range(uvaia_gpu_ctx *c, const uint4 *planes, long long tile_first, int n_tiles, int r_lo, int r_hi, int radius, int *mindist_host)
{
  const int n = r_hi - r_lo;
  if (n <= 0) return 0;
  const size_t cap = std::max<size_t>((size_t)n_tiles * 64, c->pool_pad);
  for (DevBuf<int> *b : {&c->ball.d_mindist, &c->ball.d_list, &c->ball.d_cdist}) if (int rc = b->reserve(c, cap)) return rc;
  if (int rc = c->ball.d_n.reserve(c, 1)) return rc;
  for (Event &e : c->ball.ev) if (int rc = e.make(c)) return rc;   // the four timing events
  HIPCHK(c, hipMemsetAsync(c->ball.d_n, 0, sizeof(int), c->st.stream));
  { int rc = ensure_qgather(c); if (rc) return rc; }        // the order of the columns of query->idx in the gathered words, the queries on them
  // the gathered columns of every reference of the range, written by stage 1 itself (1/7 of the range's planes for the benchmark's
  // queries); without room for them the references that go on are gathered by a pass of their own
  const size_t tile_u4 = (size_t)c->ball.NG4 * c->P * 64;
  bool fused = c->ball.fused;
  if (fused && c->ball.d_ga.reserve(c, (size_t)n_tiles * tile_u4)) { (void)hipGetLastError(); fused = false; }
  HIPCHK(c, hipEventRecord(c->ball.ev[0], c->st.stream));
#define BALL_STAGE1(A, G) hipLaunchKernelGGL((ball_stage1_kernel<A, G>), dim3((n_tiles + 3) / 4), dim3(256), 0, c->st.stream, planes, tile_first, n_tiles, c->W4, c->tab.d_cp, c->tab.d_cpm, radius, \
                                              r_lo, r_hi, c->ball.d_mindist, c->ball.d_cdist, c->ball.d_list, c->ball.d_n, c->ball.d_masks, c->ball.NH4, c->ball.NG4, c->ball.d_ga, c->n_idx_c > 0, c->n_idx_m > 0)
  if (c->acgt) { if (fused) BALL_STAGE1(true, true); else BALL_STAGE1(true, false); }
  else         { if (fused) BALL_STAGE1(false, true); else BALL_STAGE1(false, false); }
#undef BALL_STAGE1
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ball.ev[1], c->st.stream));
  int n_ask = 0;
  HIPCHK(c, hipMemcpyAsync(&n_ask, c->ball.d_n, sizeof(int), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  c->ball.asked += (unsigned long long)n_ask;
  // the references whose answer depends on the queries: their planes on the columns of query->idx gathered into dense tiles, the pair
  // scan on those, the reference's walk over the queries folded into it (kernels_ball.inc)
  if (n_ask > 0) {
    const int mt = (n_ask + 63) / 64;
    if (c->ball.d_key.cap < (size_t)mt * 64) {              // (the keys are made last: room for them is room for the tiles)
      const size_t tcap = (size_t)mt + (size_t)mt / 4 + 16;
      c->ball.d_key.release();
      if (int rc = c->ball.d_tiles.reserve(c, tcap * tile_u4)) return rc;
      if (int rc = c->ball.d_key.reserve(c, tcap * 64)) return rc;
    }
    HIPCHK(c, hipMemsetAsync(c->ball.d_key, 0xFF, (size_t)mt * 64 * sizeof(unsigned long long), c->st.stream));
    if (fused) {
      if (c->acgt) hipLaunchKernelGGL((ball_compact_kernel<3>), dim3(mt), dim3(64), 0, c->st.stream, c->ball.d_ga, c->ball.d_list, n_ask, c->ball.NG4, c->ball.d_tiles);
      else         hipLaunchKernelGGL((ball_compact_kernel<4>), dim3(mt), dim3(64), 0, c->st.stream, c->ball.d_ga, c->ball.d_list, n_ask, c->ball.NG4, c->ball.d_tiles);
    } else {
      if (c->acgt) hipLaunchKernelGGL((ball_gather_cols_kernel<3>), dim3(mt), dim3(64), 0, c->st.stream, planes, tile_first, c->W4, c->ball.d_masks, c->ball.d_list, n_ask, c->ball.NH4, c->ball.NG4, c->ball.d_tiles);
      else         hipLaunchKernelGGL((ball_gather_cols_kernel<4>), dim3(mt), dim3(64), 0, c->st.stream, planes, tile_first, c->W4, c->ball.d_masks, c->ball.d_list, n_ask, c->ball.NH4, c->ball.NG4, c->ball.d_tiles);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ball.ev[2], c->st.stream));
    constexpr int QTB = 16;
    const int n_qtiles = (c->nq + QTB - 1) / QTB;
    dim3 grid(scan_grid_size(n_qtiles, (mt + 3) / 4));
    if (c->acgt) hipLaunchKernelGGL((ball_scan_kernel<true, QTB>), grid, dim3(256), 0, c->st.stream, c->ball.d_tiles, mt, c->ball.NG4, c->ball.d_qg, c->nq, n_qtiles, c->ball.d_cdist, n_ask, radius, c->ball.d_key);
    else         hipLaunchKernelGGL((ball_scan_kernel<false, QTB>), grid, dim3(256), 0, c->st.stream, c->ball.d_tiles, mt, c->ball.NG4, c->ball.d_qg, c->nq, n_qtiles, c->ball.d_cdist, n_ask, radius, c->ball.d_key);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ball.ev[3], c->st.stream));
    hipLaunchKernelGGL(ball_finish2_kernel, dim3((n_ask + 255) / 256), dim3(256), 0, c->st.stream, c->ball.d_key, c->ball.d_list, c->ball.d_cdist, n_ask, radius, r_lo, c->ball.d_mindist);
    HIPCHK(c, hipGetLastError());
  }
  if (mindist_host) HIPCHK(c, hipMemcpyAsync(mindist_host, c->ball.d_mindist, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  // the time of each kernel of this call, for uvaia_gpu_ball_kernel_ms (the events were already waited for by the synchronisation above)
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->ball.ev[0], c->ball.ev[1]) == hipSuccess) c->ball.ms[0] += ms;
  if (n_ask > 0) {
    if (hipEventElapsedTime(&ms, c->ball.ev[1], c->ball.ev[2]) == hipSuccess) c->ball.ms[1] += ms;   // includes the read-back of the count
    if (hipEventElapsedTime(&ms, c->ball.ev[2], c->ball.ev[3]) == hipSuccess) c->ball.ms[2] += ms;
  }
  return 0;
}

int uvaia_gpu_ball(uvaia_gpu_ctx *c, const char *const *seq, int n_ref, int radius, int *mindist)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_ref < 0 || (n_ref > 0 && (!seq || !mindist))) return fail(c, UVAIA_GPU_EINVAL, "bad batch");
  if ((size_t)n_ref > c->max_pool) return fail(c, UVAIA_GPU_ESTATE, "batch of %d exceeds max_pool %zu", n_ref, c->max_pool);
  if (c->act_q0 != 0 || c->act_q1 != c->nq) return fail(c, UVAIA_GPU_ESTATE, "the radius search acts on the whole query set");
  if (n_ref == 0) return 0;
  int rc = ensure_batch_buffers(c); if (rc) return rc;
  rc = pack_rows(c, seq, nullptr, 0, nullptr, n_ref, c->batch, 0);
  if (rc) return rc;
  return ball_range(c, c->batch.planes, 0, (n_ref + 63) / 64, 0, n_ref, radius, mindist);
}

// the same over references [first, first + n) of the resident database (uvaia_gpu_db_append*): mindist[i] for reference first + i
int uvaia_gpu_ball_resident(uvaia_gpu_ctx *c, size_t first, size_t n, int radius, int *mindist)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (first + n > c->db_n) return fail(c, UVAIA_GPU_EINVAL, "range [%zu,+%zu) outside the database", first, n);
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only");
  if (c->act_q0 != 0 || c->act_q1 != c->nq) return fail(c, UVAIA_GPU_ESTATE, "the radius search acts on the whole query set");
  if (int rc = sync_scan_streams(c)) return rc;
  const size_t step = (size_t)1 << 22;                       // stage 1 needs no more than 12 bytes per reference of work space
  for (size_t a = first; a < first + n; a += step) {
    const size_t b = std::min(first + n, a + step);
    const long long tf = (long long)(a / 64);
    int rc = ball_range(c, c->db.planes, tf, (int)((b + 63) / 64 - a / 64), (int)(a - (size_t)tf * 64), (int)(b - (size_t)tf * 64), radius, mindist ? mindist + (a - first) : nullptr);
    if (rc) return rc;
  }
  return 0;
}

// the same for a batch handed in as whole tiles of the interchange form: searched where the copy lands (default mode) or from the batch
// store after import_tiles_kernel<3> (--acgt), then forgotten by the search; nothing is derived, the resident database is not touched.
// ball_range reads only the planes of its store (no side rows, no valid-site counts), so a store that holds nothing else will do.
int uvaia_gpu_ball_packed(uvaia_gpu_ctx *c, const void *planes, int n_ref, int radius, int *mindist)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_ref < 0 || (n_ref > 0 && (!planes || !mindist))) return fail(c, UVAIA_GPU_EINVAL, "bad batch");
  if ((size_t)n_ref > c->max_pool) return fail(c, UVAIA_GPU_ESTATE, "batch of %d exceeds max_pool %zu", n_ref, c->max_pool);
  if (c->act_q0 != 0 || c->act_q1 != c->nq) return fail(c, UVAIA_GPU_ESTATE, "the radius search acts on the whole query set");
  c->ball.pk_n = 0;                                               // the tiles of the previous call are about to be replaced
  if (n_ref == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t tb = uvaia_gpu_db_tile_bytes(c);
  const int n_tiles = (n_ref + 63) / 64;
  if (int rc = c->ball.d_pk.reserve(c, (c->pool_pad / 64) * tb / sizeof(uint4))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->ball.d_pk, planes, (size_t)n_tiles * tb, hipMemcpyHostToDevice, c->st.stream));
  int rc;
  if (c->acgt) {
    rc = ensure_batch_buffers(c); if (rc) return rc;
    hipLaunchKernelGGL((import_tiles_kernel<3>), dim3((unsigned)n_tiles), dim3(256), 0, c->st.stream, c->ball.d_pk, c->W4, c->batch.planes, 0LL, c->batch.tot);
    HIPCHK(c, hipGetLastError());
    rc = ball_range(c, c->batch.planes, 0, n_tiles, 0, n_ref, radius, mindist);
  } else rc = ball_range(c, c->ball.d_pk, 0, n_tiles, 0, n_ref, radius, mindist);      // the four planes as they came are a store's own form
  if (rc) return rc;
  c->ball.pk_n = n_ref;
  return 0;
}

// text of references index[0..n) of `count` references held as four-plane tiles at `tiles`, rows + k * pitch; see unpack_rows_kernel.
// what / first: how the two entries name the tiles in their error texts.  ev (nullable): two events that bracket every kernel launch
// of the call, the elapsed time of each pair is added to *ms.
static int unpack_rows_from(uvaia_gpu_ctx *c, const uint4 *tiles, int count, const char *what, const char *first, const int *index, int n, char *rows, size_t pitch,
                            Event *ev = nullptr, double *ms = nullptr)
{
  if (n < 0 || (n > 0 && (!index || !rows))) return fail(c, UVAIA_GPU_EINVAL, "bad selection");
  if (pitch < (size_t)c->nchar) return fail(c, UVAIA_GPU_EINVAL, "pitch %zu is below the %d sites of a row", pitch, c->nchar);
  if (!count) return fail(c, UVAIA_GPU_ESTATE, "no %s to unpack: %s comes first", what, first);
  for (int k = 0; k < n; k++)
    if (index[k] < 0 || index[k] >= count) return fail(c, UVAIA_GPU_EINVAL, "index[%d] = %d lies outside the last %s of %d", k, index[k], what, count);
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t dpitch = ((size_t)c->nchar + 15) / 16 * 16;
  const size_t chunk = std::min((size_t)n, c->pool_pad);    // a selection may repeat references: longer ones go in rounds of a pool
  if (int rc = c->ball.d_rows.reserve(c, chunk * dpitch)) return rc;
  if (int rc = c->ball.d_row_idx.reserve(c, chunk)) return rc;
  for (size_t a = 0; a < (size_t)n; a += chunk) {
    const size_t m = std::min(chunk, (size_t)n - a);
    HIPCHK(c, hipMemcpyAsync(c->ball.d_row_idx, index + a, m * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
    if (ev) HIPCHK(c, hipEventRecord(ev[0], c->st.stream));
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)m), dim3(256), 0, c->st.stream, tiles, c->W4, c->nchar, c->ball.d_row_idx, c->ball.d_rows, dpitch);
    HIPCHK(c, hipGetLastError());
    if (ev) HIPCHK(c, hipEventRecord(ev[1], c->st.stream));
    // one copy for all rows of the round: straight when the caller's rows have the staging pitch, strided otherwise
    if (pitch == dpitch) HIPCHK(c, hipMemcpyAsync(rows + a * pitch, c->ball.d_rows, m * dpitch, hipMemcpyDeviceToHost, c->st.stream));
    else HIPCHK(c, hipMemcpy2DAsync(rows + a * pitch, pitch, c->ball.d_rows, dpitch, (size_t)c->nchar, m, hipMemcpyDeviceToHost, c->st.stream));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    if (ev && ms) { float t = 0.f; if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) *ms += t; }
  }
  return 0;
}

// text of references index[0..n) of the last uvaia_gpu_ball_packed batch
int uvaia_gpu_unpack_rows(uvaia_gpu_ctx *c, const int *index, int n, char *rows, size_t pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  return unpack_rows_from(c, c->ball.d_pk, c->ball.pk_n, "packed batch", "uvaia_gpu_ball_packed", index, n, rows, pitch);
}

// references the last radius searches sent on to the queries (since the last call with reset != 0)
void uvaia_gpu_ball_kernel_ms(uvaia_gpu_ctx *c, double out[3], int reset)
{
  if (!c) return;
  for (int i = 0; i < 3; i++) { out[i] = c->ball.ms[i]; if (reset) c->ball.ms[i] = 0.; }
}
unsigned long long uvaia_gpu_ball_asked(uvaia_gpu_ctx *c, int reset) { if (!c) return 0; const unsigned long long v = c->ball.asked; if (reset) c->ball.asked = 0; return v; }


}  // extern "C"
