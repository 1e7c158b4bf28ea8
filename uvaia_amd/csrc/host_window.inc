// host_window.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the windowed search over a packed database that does
// not fit device memory: two staging slots of whole file tiles filled by a copy stream, the load of a selection of their lanes into the
// resident store (select_tiles_kernel), the text of a loaded window.  The search itself is uvaia_gpu_search_resident, window after window:
// its state (heaps, tolerances) lives in the context and ordinal0 gives the stream position.

extern "C" {

static_assert(AMB_ROW == 64, "select_tiles_kernel moves a side row with one wave");

// tiles each of the two staging slots holds room for: slot 1's planes are the last array uvaia_gpu_db_stage_reserve makes
static size_t stage_tiles(const uvaia_gpu_ctx *c) { return c->win.stage[1].planes.cap / ((size_t)c->W4 * 4 * 64); }

size_t uvaia_gpu_free_bytes(uvaia_gpu_ctx *c)
{
  if (!c || hipSetDevice(c->device) != hipSuccess) return 0;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return free_b;
}

int uvaia_gpu_db_stage_reserve(uvaia_gpu_ctx *c, size_t n_tiles)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: staged windows need a plain context");
  if (n_tiles < 1 || n_tiles > (size_t)(0x7FFFFFFF / 64)) return fail(c, UVAIA_GPU_EINVAL, "staging capacity of %zu tiles", n_tiles);
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->win.copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->win.copy_stream.s, hipStreamNonBlocking));
  for (auto &sl : c->win.stage) {
    if (int rc = sl.copied.make(c, hipEventDisableTiming)) return rc;
    if (int rc = sl.read.make(c, hipEventDisableTiming)) return rc;
  }
  if (n_tiles <= stage_tiles(c)) return 0;
  HIPCHK(c, hipStreamSynchronize(c->win.copy_stream));          // nothing may still use the slots that go
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  for (auto &sl : c->win.stage) { sl.planes.release(); sl.nonn.release(); sl.side.release(); sl.n_tiles = 0; sl.read_recorded = false; }    // both first: the capacity is slot 1's
  for (auto &sl : c->win.stage) {
    if (int rc = sl.nonn.reserve(c, n_tiles * 64)) return rc;
    if (int rc = sl.side.reserve(c, n_tiles * 64 * AMB_ROW)) return rc;
    if (int rc = sl.planes.reserve(c, n_tiles * (size_t)c->W4 * 4 * 64)) return rc;
  }
  return 0;
}

// what load_staged and append_staged refuse before anything is touched
static int check_staged(uvaia_gpu_ctx *c, int slot, const int *sel, int n_ref)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: staged windows need a plain context");
  if (slot < 0 || slot > 1) return fail(c, UVAIA_GPU_EINVAL, "staging slot %d: there are slots 0 and 1", slot);
  if (n_ref < 0) return fail(c, UVAIA_GPU_EINVAL, "negative count");
  const long long staged = (long long)c->win.stage[slot].n_tiles * 64;
  if (n_ref > 0 && !staged) return fail(c, UVAIA_GPU_ESTATE, "staging slot %d holds no tiles: uvaia_gpu_db_stage_packed comes first", slot);
  if (!sel && n_ref > staged) return fail(c, UVAIA_GPU_EINVAL, "%d references asked of the %lld staged in slot %d", n_ref, staged, slot);
  if (sel) for (int k = 0; k < n_ref; k++)
    if (sel[k] < 0 || sel[k] >= staged) return fail(c, UVAIA_GPU_EINVAL, "sel[%d] = %d lies outside the %lld references staged in slot %d", k, sel[k], staged, slot);
  return 0;
}

// sel (may be NULL) to the device, on the context's stream
static int upload_sel(uvaia_gpu_ctx *c, const int *sel, int n_ref)
{
  if (!sel) return 0;
  if (int rc = c->win.d_sel.reserve(c, (size_t)n_ref)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->win.d_sel, sel, (size_t)n_ref * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
  return 0;
}

// the end of a load: the third event, the wait, the device time of the selection and of what followed it
static int finish_staged(uvaia_gpu_ctx *c)
{
  HIPCHK(c, hipEventRecord(c->win.ev[2], c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));     // scans start on other streams: the packed and derived planes must be complete
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->win.ev[0], c->win.ev[1]) == hipSuccess) c->win.ms[0] += ms;
  if (hipEventElapsedTime(&ms, c->win.ev[1], c->win.ev[2]) == hipSuccess) c->win.ms[1] += ms;
  return 0;
}

int uvaia_gpu_db_load_staged(uvaia_gpu_ctx *c, int slot, const int *sel, int n_ref)
{
  if (int rc = check_staged(c, slot, sel, n_ref)) return rc;
  auto &sl = c->win.stage[slot];
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = uvaia_gpu_db_clear(c); if (rc) return rc; }
  c->win.n = 0;
  if (n_ref == 0) return 0;
  if ((size_t)n_ref > c->db_cap) { int rc = uvaia_gpu_db_reserve(c, (size_t)n_ref); if (rc) return rc; }
  const size_t n_tiles = ((size_t)n_ref + 63) / 64;
  bool grown = false;
  if (int rc = win_image_room(c, n_tiles, &grown)) return rc;
  if (int rc = upload_sel(c, sel, n_ref)) return rc;
  for (Event &e : c->win.ev) if (int rc = e.make(c)) return rc;
  HIPCHK(c, hipStreamWaitEvent(c->st.stream, sl.copied, 0));
  uint4 *four = c->acgt ? c->win.d_four.p : c->db.planes.p;
  HIPCHK(c, hipEventRecord(c->win.ev[0], c->st.stream));
  hipLaunchKernelGGL(select_tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->st.stream, sl.planes, sl.nonn, c->acgt ? (const int *)nullptr : sl.side, sel ? c->win.d_sel : (const int *)nullptr, n_ref, c->W4,
                     four, c->db.nonn, c->acgt ? (int *)nullptr : c->db.amb);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->win.ev[1], c->st.stream));
  HIPCHK(c, hipEventRecord(sl.read, c->st.stream)); sl.read_recorded = true;
  // from here on as uvaia_gpu_db_append_packed: re-coding (--acgt) and totals, the checks on what came from outside, the derived planes
  if (int rc = db_import_tiles(c, c->win.d_four, 0, n_tiles)) return rc;
  if (int rc = db_sanitise_import(c, 0, n_tiles * 64)) return rc;
  { int rc = derive_rows(c, c->db, 0, (int)(n_tiles * 64)); if (rc) return rc; }
  if (int rc = finish_staged(c)) return rc;
  db_commit(c, (size_t)n_ref, n_ref);
  return 0;
}

int uvaia_gpu_db_stage_packed_at(uvaia_gpu_ctx *c, int slot, size_t tile_offset, const void *planes, const int *non_n, const int *side_rows, int n_tiles)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: staged windows need a plain context");
  if (slot < 0 || slot > 1) return fail(c, UVAIA_GPU_EINVAL, "staging slot %d: there are slots 0 and 1", slot);
  if (n_tiles < 0 || (n_tiles > 0 && (!planes || !non_n || (!c->acgt && !side_rows)))) return fail(c, UVAIA_GPU_EINVAL, "NULL packed arrays");
  if (tile_offset > stage_tiles(c) || (size_t)n_tiles > stage_tiles(c) - tile_offset)
    return fail(c, UVAIA_GPU_ESTATE, "%d tiles at tile %zu exceed the staging capacity of %zu: call uvaia_gpu_db_stage_reserve first", n_tiles, tile_offset, stage_tiles(c));
  HIPCHK(c, hipSetDevice(c->device));
  auto &sl = c->win.stage[slot];
  const size_t before = tile_offset ? (size_t)sl.n_tiles : 0;      // a piece at tile 0 starts the slot afresh
  sl.n_tiles = 0;
  if (sl.read_recorded) HIPCHK(c, hipStreamWaitEvent(c->win.copy_stream, sl.read, 0));       // the load that still reads the slot's previous tiles
  if (n_tiles) {
    const size_t tb = uvaia_gpu_db_tile_bytes(c), nt = (size_t)n_tiles;
    HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char *>(sl.planes.p) + tile_offset * tb, planes, nt * tb, hipMemcpyHostToDevice, c->win.copy_stream));
    HIPCHK(c, hipMemcpyAsync(sl.nonn + tile_offset * 64, non_n, nt * 64 * sizeof(int), hipMemcpyHostToDevice, c->win.copy_stream));
    if (!c->acgt) HIPCHK(c, hipMemcpyAsync(sl.side + tile_offset * 64 * AMB_ROW, side_rows, nt * 64 * AMB_ROW * sizeof(int), hipMemcpyHostToDevice, c->win.copy_stream));
  }
  HIPCHK(c, hipEventRecord(sl.copied, c->win.copy_stream));        // the copy stream runs in order: this one covers the earlier pieces too
  sl.n_tiles = (int)std::max(before, tile_offset + (size_t)n_tiles);
  return 0;
}

// device time of the expansion queued last, once it has run (the events are recorded anew by every uvaia_gpu_db_stage_compact_at)
static void compact_harvest(uvaia_gpu_ctx *c)
{
  auto &k = c->win.compact;
  if (!k.timed) return;
  k.timed = false;
  if (hipEventSynchronize(k.ev[2]) != hipSuccess) { (void)hipGetLastError(); return; }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, k.ev[0], k.ev[1]) == hipSuccess) k.ms[0] += ms;
  if (hipEventElapsedTime(&ms, k.ev[1], k.ev[2]) == hipSuccess) k.ms[1] += ms;
}

int uvaia_gpu_db_stage_compact_at(uvaia_gpu_ctx *c, int slot, size_t tile_offset, const void *base, const uint64_t *head_idx, const uint32_t *heads,
                                  const uint64_t *lit_idx, const void *lits, const int *non_n, int n_tiles)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: staged windows need a plain context");
  if (slot < 0 || slot > 1) return fail(c, UVAIA_GPU_EINVAL, "staging slot %d: there are slots 0 and 1", slot);
  if (n_tiles < 0 || (n_tiles > 0 && (!base || !head_idx || !lit_idx || !non_n))) return fail(c, UVAIA_GPU_EINVAL, "NULL compact arrays");
  if (tile_offset > stage_tiles(c) || (size_t)n_tiles > stage_tiles(c) - tile_offset)
    return fail(c, UVAIA_GPU_ESTATE, "%d tiles at tile %zu exceed the staging capacity of %zu: call uvaia_gpu_db_stage_reserve first", n_tiles, tile_offset, stage_tiles(c));
  const size_t nt = (size_t)n_tiles, lanes = nt * 64;
  uint64_t nh = 0, nl = 0;
  if (n_tiles) {
    if (head_idx[lanes] < head_idx[0] || lit_idx[lanes] < lit_idx[0]) return fail(c, UVAIA_GPU_EINVAL, "compact index arrays that decrease");
    nh = head_idx[lanes] - head_idx[0]; nl = lit_idx[lanes] - lit_idx[0];
    if ((nh && !heads) || (nl && !lits)) return fail(c, UVAIA_GPU_EINVAL, "NULL compact arrays");
  }
  HIPCHK(c, hipSetDevice(c->device));
  auto &sl = c->win.stage[slot];
  auto &k = c->win.compact;
  const size_t before = tile_offset ? (size_t)sl.n_tiles : 0;      // a piece at tile 0 starts the slot afresh
  sl.n_tiles = 0;
  if (sl.read_recorded) HIPCHK(c, hipStreamWaitEvent(c->win.copy_stream, sl.read, 0));       // the load that still reads the slot's previous tiles
  if (n_tiles) {
    compact_harvest(c);
    for (Event &e : k.ev) if (int rc = e.make(c)) return rc;
    // the copy stream runs in order: the buffers are free again once the expansion queued before has read them (a buffer that grows is
    // released by a call that waits for the device)
    const size_t W4 = (size_t)c->W4;
    if (int rc = k.base.reserve(c, W4 * 4)) return rc;
    if (int rc = k.hidx.reserve(c, lanes + 1)) return rc;
    if (int rc = k.lidx.reserve(c, lanes + 1)) return rc;
    if (int rc = k.heads.reserve(c, (size_t)nh + 1)) return rc;
    if (int rc = k.lits.reserve(c, (size_t)nl * 4 + 4)) return rc;
    hipStream_t cs = c->win.copy_stream;
    HIPCHK(c, hipMemcpyAsync(k.base, base, W4 * 4 * sizeof(uint4), hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipMemcpyAsync(k.hidx, head_idx, (lanes + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipMemcpyAsync(k.lidx, lit_idx, (lanes + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, cs));
    if (nh) HIPCHK(c, hipMemcpyAsync(k.heads, heads + head_idx[0], (size_t)nh * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
    if (nl) HIPCHK(c, hipMemcpyAsync(k.lits, static_cast<const char *>(lits) + lit_idx[0] * 16, (size_t)nl * 16, hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipMemcpyAsync(sl.nonn + tile_offset * 64, non_n, lanes * sizeof(int), hipMemcpyHostToDevice, cs));
    uint4 *dst = sl.planes.p + tile_offset * W4 * 4 * 64;
    HIPCHK(c, hipEventRecord(k.ev[0], cs));
    hipLaunchKernelGGL(expand_tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, cs, k.base, k.hidx, k.heads, (unsigned long long)nh, k.lidx, k.lits, (unsigned long long)nl, c->W4, dst);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(k.ev[1], cs));
    if (!c->acgt) {                                               // (an --acgt context keeps no side rows)
      hipLaunchKernelGGL(side_rows_staged_kernel, dim3((unsigned)n_tiles), dim3(64), 0, cs, dst, c->W4, sl.side + tile_offset * 64 * AMB_ROW);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(k.ev[2], cs));
    k.timed = true;
  }
  HIPCHK(c, hipEventRecord(sl.copied, c->win.copy_stream));        // the copy stream runs in order: this one covers the earlier pieces too
  sl.n_tiles = (int)std::max(before, tile_offset + (size_t)n_tiles);
  return 0;
}

void uvaia_gpu_compact_ms(uvaia_gpu_ctx *c, double out[2], int reset)
{
  if (!c) return;
  if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return; }
  compact_harvest(c);
  for (int i = 0; i < 2; i++) { out[i] = c->win.compact.ms[i]; if (reset) c->win.compact.ms[i] = 0.; }
}

int uvaia_gpu_db_stage_packed(uvaia_gpu_ctx *c, int slot, const void *planes, const int *non_n, const int *side_rows, int n_tiles)
{
  return uvaia_gpu_db_stage_packed_at(c, slot, 0, planes, non_n, side_rows, n_tiles);
}

int uvaia_gpu_db_append_staged(uvaia_gpu_ctx *c, int slot, const int *sel, int n_ref)
{
  if (int rc = check_staged(c, slot, sel, n_ref)) return rc;
  auto &sl = c->win.stage[slot];
  if (n_ref == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = db_make_room(c, (size_t)n_ref)) return rc;
  const size_t n0 = c->db_n, n1 = n0 + (size_t)n_ref;
  const long long t0 = (long long)(n0 / 64), t1 = (long long)((n1 - 1) / 64);
  // the four-plane image the text is decoded from (uvaia_gpu_db_unpack_rows): the resident planes themselves in a default-mode context; an
  // --acgt context keeps it next to them, and it is whole as long as every resident reference came through load_staged / append_staged
  bool image = n1 <= 0x7FFFFFFFu && (!c->acgt || n0 == 0 || (c->win.n > 0 && (size_t)c->win.n == n0)), grown = false;
  if (int rc = win_image_room(c, c->db_cap / 64 + 1, &grown)) return rc;
  if (grown && n0) image = false;                       // (what it held goes with the old array)
  if (n0 % 64) { if (int rc = sync_scan_streams(c)) return rc; }      // the derived planes of the first tile are rebuilt: no scan may still read them
  if (int rc = upload_sel(c, sel, n_ref)) return rc;
  for (Event &e : c->win.ev) if (int rc = e.make(c)) return rc;
  HIPCHK(c, hipStreamWaitEvent(c->st.stream, sl.copied, 0));
  HIPCHK(c, hipEventRecord(c->win.ev[0], c->st.stream));
  const unsigned nblk = (unsigned)(t1 - t0 + 1);
  const int *d_sel = sel ? c->win.d_sel : (const int *)nullptr;
  if (c->acgt) hipLaunchKernelGGL((append_lanes_kernel<3>), dim3(nblk), dim3(256), 0, c->st.stream, sl.planes, sl.nonn, (const int *)nullptr, d_sel, (long long)n0, n_ref, c->W4,
                                  c->db.planes, c->win.d_four, t0, c->db.nonn, (int *)nullptr, c->db.tot);
  else         hipLaunchKernelGGL((append_lanes_kernel<4>), dim3(nblk), dim3(256), 0, c->st.stream, sl.planes, sl.nonn, sl.side, d_sel, (long long)n0, n_ref, c->W4,
                                  c->db.planes, (uint4 *)nullptr, t0, c->db.nonn, c->db.amb, c->db.tot);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->win.ev[1], c->st.stream));
  HIPCHK(c, hipEventRecord(sl.read, c->st.stream)); sl.read_recorded = true;
  // as uvaia_gpu_db_append_packed, for the rows added: the checks on what came from outside, the derived planes of their tiles
  if (int rc = db_sanitise_import(c, n0, (size_t)n_ref)) return rc;
  { int rc = derive_rows(c, c->db, (long long)n0, n_ref); if (rc) return rc; }
  if (int rc = finish_staged(c)) return rc;
  db_commit(c, n1, image ? (int)n1 : 0);
  return 0;
}

// text of references index[0..n) of the window loaded last (positions within the window)
int uvaia_gpu_db_unpack_rows(uvaia_gpu_ctx *c, const int *index, int n, char *rows, size_t pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  const int count = (c->win.n && (size_t)c->win.n == c->db_n) ? c->win.n : 0;     // (the database changed since the load: the window is gone)
  for (int i = 3; i < 5; i++) if (int rc = c->win.ev[i].make(c)) return rc;
  return unpack_rows_from(c, c->acgt ? c->win.d_four : c->db.planes, count, "loaded window", "uvaia_gpu_db_load_staged", index, n, rows, pitch, c->win.ev + 3, &c->win.ms[2]);
}

// text of lanes index[0..n) of staging slot `slot` (positions within the slot, as sel of load_staged), decoded where the slot lies: the
// resident database, the loaded window and the search state are not touched
int uvaia_gpu_db_stage_unpack_rows(uvaia_gpu_ctx *c, int slot, const int *index, int n, char *rows, size_t pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps its own pieces only: staged windows need a plain context");
  if (slot < 0 || slot > 1) return fail(c, UVAIA_GPU_EINVAL, "staging slot %d: there are slots 0 and 1", slot);
  auto &sl = c->win.stage[slot];
  const int count = sl.n_tiles * 64;                       // (stage_reserve bounds a slot by what an int counts)
  if (count) {
    HIPCHK(c, hipSetDevice(c->device));
    for (Event &e : c->win.slot_ev) if (int rc = e.make(c)) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->st.stream, sl.copied, 0));
  }
  char what[32];
  snprintf(what, sizeof what, "staging slot %d", slot);
  const int rc = unpack_rows_from(c, sl.planes, count, what, "uvaia_gpu_db_stage_packed", index, n, rows, pitch, c->win.slot_ev, &c->win.slot_ms);
  if (rc || n == 0) return rc;
  HIPCHK(c, hipEventRecord(sl.read, c->st.stream)); sl.read_recorded = true;      // the next stage into the slot waits for the decode
  return 0;
}

double uvaia_gpu_stage_unpack_ms(uvaia_gpu_ctx *c, int reset)
{
  if (!c) return 0.;
  const double v = c->win.slot_ms;
  if (reset) c->win.slot_ms = 0.;
  return v;
}

void uvaia_gpu_window_ms(uvaia_gpu_ctx *c, double out[3], int reset)
{
  if (!c) return;
  for (int i = 0; i < 3; i++) { out[i] = c->win.ms[i]; if (reset) c->win.ms[i] = 0.; }
}

}  // extern "C"
