// host_rows.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): rows that are already in device memory on their way into the
// resident database and the packed database file: census, append without host staging, exception records, dropping exported tiles.

namespace {

// A block of rows handed in by device pointer: it must be device memory of the context's device and rows 0 .. last_row must lie inside its
// allocation (rows_block.h has the check).
int rows_check_block(uvaia_gpu_ctx *c, const void *d_rows, size_t pitch, long long last_row)
{
  char msg[256];
  return rows_block_ok(d_rows, pitch, c->nchar, c->device, last_row, msg, sizeof msg) ? 0 : fail(c, UVAIA_GPU_EINVAL, "%s", msg);
}

// largest row a selection names (row_index NULL: rows 0 .. n_sel - 1); negative entries are refused
int rows_last_selected(uvaia_gpu_ctx *c, const int *row_index, int n_sel, long long *last)
{
  long long mx = row_index ? -1 : (long long)n_sel - 1;
  if (row_index) for (int k = 0; k < n_sel; k++) { if (row_index[k] < 0) return fail(c, UVAIA_GPU_EINVAL, "row_index[%d] = %d is negative", k, row_index[k]); mx = std::max<long long>(mx, row_index[k]); }
  *last = mx;
  return 0;
}

int rows_upload_selection(uvaia_gpu_ctx *c, const int *row_index, int n_sel)
{
  if (int rc = c->rows.d_sel.reserve(c, (size_t)n_sel)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->rows.d_sel, row_index, (size_t)n_sel * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
  return 0;
}

// timing of the three kernels: pair i of the event pool brackets one launch, read after the stream has been waited for
int rows_event_pair(uvaia_gpu_ctx *c, size_t i, Event **ev)
{
  while (c->rows.evs.size() < 2 * (i + 1)) { Event e; if (int rc = e.make(c)) return rc; c->rows.evs.push_back(std::move(e)); }
  *ev = &c->rows.evs[2 * i];
  return 0;
}
int rows_add_ms(uvaia_gpu_ctx *c, int which, size_t n_pairs)
{
  for (size_t i = 0; i < n_pairs; i++) { float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, c->rows.evs[2 * i], c->rows.evs[2 * i + 1])); c->rows.ms[which] += ms; }
  return 0;
}

}  // namespace

extern "C" {

int uvaia_gpu_rows_census(uvaia_gpu_ctx *c, const void *d_rows, size_t pitch, int n, int *non_n, int *n_exc)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n < 0 || (n > 0 && (!non_n || !n_exc))) return fail(c, UVAIA_GPU_EINVAL, "bad census arguments");
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = rows_check_block(c, d_rows, pitch, (long long)n - 1)) return rc;
  const size_t need = 2 * (size_t)n + 1;               // valid sites, records, and the bad-byte flag behind them: one copy back
  if (int rc = c->rows.d_cnt.reserve(c, need)) return rc;
  int *d_flag = c->rows.d_cnt + 2 * (size_t)n;
  HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(int), c->st.stream));
  Event *ev; if (int rc = rows_event_pair(c, 0, &ev)) return rc;
  HIPCHK(c, hipEventRecord(ev[0], c->st.stream));
  const uint8_t *rows = reinterpret_cast<const uint8_t *>(d_rows);
  if ((uint32_t)c->nchar > c->rows.run_cut) hipLaunchKernelGGL((rows_census_kernel<true>), dim3((unsigned)n), dim3(ROWS_TPB), 0, c->st.stream, rows, pitch, c->nchar, c->rows.run_cut, c->rows.d_cnt, c->rows.d_cnt + n, d_flag);
  else                                 hipLaunchKernelGGL((rows_census_kernel<false>), dim3((unsigned)n), dim3(ROWS_TPB), 0, c->st.stream, rows, pitch, c->nchar, c->rows.run_cut, c->rows.d_cnt, c->rows.d_cnt + n, d_flag);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(ev[1], c->st.stream));
  c->rows.host.resize(need);
  HIPCHK(c, hipMemcpyAsync(c->rows.host.data(), c->rows.d_cnt, need * sizeof(int), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (int rc = rows_add_ms(c, 0, 1)) return rc;
  memcpy(non_n, c->rows.host.data(), (size_t)n * sizeof(int));
  memcpy(n_exc, c->rows.host.data() + n, (size_t)n * sizeof(int));
  if (c->rows.host[2 * (size_t)n]) return fail(c, UVAIA_GPU_EALPHABET, "a reference sequence holds a byte outside ACGT / MRWSYKVHDB / NX-?O.");
  return 0;
}

int uvaia_gpu_db_append_device(uvaia_gpu_ctx *c, const void *d_rows, size_t pitch, const int *row_index, int n_sel, const int *non_n)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_sel < 0) return fail(c, UVAIA_GPU_EINVAL, "negative count");
  if (n_sel == 0) return 0;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard takes its references from the host (uvaia_gpu_db_append)");
  HIPCHK(c, hipSetDevice(c->device));
  long long last = -1;
  if (int rc = rows_last_selected(c, row_index, n_sel, &last)) return rc;
  if (int rc = rows_check_block(c, d_rows, pitch, last)) return rc;
  if (int rc = db_make_room(c, (size_t)n_sel)) return rc;
  if (row_index) { if (int rc = rows_upload_selection(c, row_index, n_sel)) return rc; }
  const TileStore &s = c->db;
  const uint8_t *rows = reinterpret_cast<const uint8_t *>(d_rows);
  size_t pairs = 0;
  // the gather fills the device half of the staging buffers the host path fills over PCIe, pack_refs_kernel reads it as it reads that
  for (int done = 0, k = 0; done < n_sel; done += PACK_CHUNK, k ^= 1) {
    const int m = std::min(PACK_CHUNK, n_sel - done);
    uint8_t *ds = c->d_stage + (size_t)k * PACK_CHUNK * c->pitch;
    Event *ev; if (int rc = rows_event_pair(c, pairs, &ev)) return rc;
    HIPCHK(c, hipEventRecord(ev[0], c->st.stream));
    hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)m), dim3(ROWS_TPB), 0, c->st.stream, rows, pitch, c->nchar, row_index ? c->rows.d_sel : (const int *)nullptr, done, ds, c->pitch);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[1], c->st.stream));
    pairs++;
    if (int rc = launch_pack_chunk(c, ds, m, s, (long long)c->db_n + done, non_n ? non_n + done : nullptr)) return rc;
  }
  if (int rc = db_canonical_side_rows(c, (long long)c->db_n, n_sel, false)) return rc;      // as uvaia_gpu_db_append leaves them; the wait is the one below
  { int rc = derive_rows(c, s, (long long)c->db_n, n_sel); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));          // the caller may overwrite its rows, scans may start on another stream
  if (int rc = rows_add_ms(c, 1, pairs)) return rc;
  if (int rc = take_pack_error(c)) return rc;
  db_commit(c, c->db_n + (size_t)n_sel, 0);
  return 0;
}

int uvaia_gpu_rows_exceptions(uvaia_gpu_ctx *c, const void *d_rows, size_t pitch, const int *row_index, int n_sel, const uint64_t *offsets, void *exc_out)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_sel < 0 || (n_sel > 0 && !offsets)) return fail(c, UVAIA_GPU_EINVAL, "bad selection");
  if (n_sel == 0) return 0;
  for (int k = 0; k < n_sel; k++) if (offsets[k + 1] < offsets[k]) return fail(c, UVAIA_GPU_EINVAL, "offsets[%d] decreases", k + 1);
  const uint64_t first = offsets[0], total = offsets[n_sel];
  if (total > first && !exc_out) return fail(c, UVAIA_GPU_EINVAL, "NULL record array");
  HIPCHK(c, hipSetDevice(c->device));
  long long last = -1;
  if (int rc = rows_last_selected(c, row_index, n_sel, &last)) return rc;
  if (int rc = rows_check_block(c, d_rows, pitch, last)) return rc;
  if (row_index) { if (int rc = rows_upload_selection(c, row_index, n_sel)) return rc; }
  if (int rc = c->rows.d_off.reserve(c, (size_t)n_sel + 1)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->rows.d_off, offsets, ((size_t)n_sel + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, c->st.stream));
  const size_t need = (size_t)total + 1;               // the records, and the flag behind them: one copy back
  if (int rc = c->rows.d_exc.reserve(c, need)) return rc;
  int *d_flag = reinterpret_cast<int *>(c->rows.d_exc + total);
  HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(uint2), c->st.stream));
  Event *ev; if (int rc = rows_event_pair(c, 0, &ev)) return rc;
  HIPCHK(c, hipEventRecord(ev[0], c->st.stream));
  const uint8_t *rows = reinterpret_cast<const uint8_t *>(d_rows);
  const int *sel = row_index ? c->rows.d_sel : nullptr;
  if ((uint32_t)c->nchar > c->rows.run_cut) hipLaunchKernelGGL((rows_fill_exceptions_kernel<true>), dim3((unsigned)n_sel), dim3(ROWS_TPB), 0, c->st.stream, rows, pitch, c->nchar, c->rows.run_cut, sel, c->rows.d_off, c->rows.d_exc, d_flag);
  else                                 hipLaunchKernelGGL((rows_fill_exceptions_kernel<false>), dim3((unsigned)n_sel), dim3(ROWS_TPB), 0, c->st.stream, rows, pitch, c->nchar, c->rows.run_cut, sel, c->rows.d_off, c->rows.d_exc, d_flag);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(ev[1], c->st.stream));
  c->rows.exc_host.resize((size_t)(total - first) + 1);
  HIPCHK(c, hipMemcpyAsync(c->rows.exc_host.data(), c->rows.d_exc + first, c->rows.exc_host.size() * sizeof(uint2), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (int rc = rows_add_ms(c, 2, 1)) return rc;
  if (c->rows.exc_host.back().x) return fail(c, UVAIA_GPU_EINVAL, "the offsets do not hold the exception records of these rows (take them from uvaia_gpu_rows_census)");
  if (total > first) memcpy(reinterpret_cast<char *>(exc_out) + first * sizeof(uint2), c->rows.exc_host.data(), (size_t)(total - first) * sizeof(uint2));
  return 0;
}

int uvaia_gpu_db_drop_tiles(uvaia_gpu_ctx *c, size_t n_tiles)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: tiles are dropped from a plain context");
  const size_t have = (c->db_n + 63) / 64;
  if (n_tiles > have) return fail(c, UVAIA_GPU_EINVAL, "%zu tiles to drop, the database holds %zu", n_tiles, have);
  if (n_tiles == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = settle_derive(c); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  if (int rc = sync_scan_streams(c)) return rc;
  const size_t rest = c->db_n > n_tiles * 64 ? c->db_n - n_tiles * 64 : 0, rest_tiles = (rest + 63) / 64;
  const size_t pw = (size_t)c->W4 * c->P * 64;         // uint4 per tile
  for (size_t t = 0; t < rest_tiles; t++) {            // towards the front, tile by tile: a copy never overlaps itself
    const size_t f = n_tiles + t;
    HIPCHK(c, hipMemcpyAsync(c->db.planes + t * pw, c->db.planes + f * pw, pw * sizeof(uint4), hipMemcpyDeviceToDevice, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(c->db.nonn + t * 64, c->db.nonn + f * 64, 64 * sizeof(int), hipMemcpyDeviceToDevice, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(c->db.tot + t * 64, c->db.tot + f * 64, 64 * sizeof(int), hipMemcpyDeviceToDevice, c->st.stream));
    HIPCHK(c, hipMemcpyAsync(c->db.amb + t * 64 * AMB_ROW, c->db.amb + f * 64 * AMB_ROW, (size_t)64 * AMB_ROW * sizeof(int), hipMemcpyDeviceToDevice, c->st.stream));
  }
  const size_t z = have - rest_tiles;                  // lanes past the last reference must read as zero planes (uvaia_gpu_db_clear)
  HIPCHK(c, hipMemsetAsync(c->db.planes + rest_tiles * pw, 0, z * pw * sizeof(uint4), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.nonn + rest_tiles * 64, 0, z * 64 * sizeof(int), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.tot + rest_tiles * 64, 0, z * 64 * sizeof(int), c->st.stream));
  HIPCHK(c, hipMemsetAsync(c->db.amb + rest_tiles * 64 * AMB_ROW, 0, z * 64 * AMB_ROW * sizeof(int), c->st.stream));
  if (c->state.d_entered) HIPCHK(c, hipMemsetAsync(c->state.d_entered, 0, std::min(c->state.d_entered.cap, have * 64), c->st.stream));
  c->db_n = rest; c->db_gen++;
  c->win.n = 0;                                        // the four-plane image of a window is not moved with the tiles
  { int rc = derive_rows(c, c->db, 0, (int)rest); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

int uvaia_gpu_rows_set_run_cut(uvaia_gpu_ctx *c, unsigned cut)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (cut > ROWS_RUN_CUT) return fail(c, UVAIA_GPU_EINVAL, "a record holds run lengths up to %u", ROWS_RUN_CUT);
  c->rows.run_cut = cut ? cut : ROWS_RUN_CUT;
  return 0;
}

void uvaia_gpu_rows_kernel_ms(uvaia_gpu_ctx *c, double out[3], int reset)
{
  if (!c) return;
  if (out) for (int i = 0; i < 3; i++) out[i] = c->rows.ms[i];
  if (reset) c->rows.ms[0] = c->rows.ms[1] = c->rows.ms[2] = 0.;
}

}  // extern "C"
