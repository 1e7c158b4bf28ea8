// host_pairs.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): all pairs of the resident database against each other:
// the checks, the cut of a rectangle into launches, the copies back, the list of the pairs within a distance, and the single-linkage
// clusters within a distance (a forest on the device: begin, link, labels).

namespace {

// One launch covers at most this rectangle: the counters of a launch (32 MiB as distances, 160 MiB as five counters), its list and the row
// records of a band (a few tens of MiB at 30 000 columns) are all the working memory, whatever the database holds.
constexpr size_t PAIRS_LAUNCH_ROWS = 1024, PAIRS_LAUNCH_COLS = 8192;
constexpr int PAIRS_SNP_RT = 32, PAIRS_SNP_RT_ALT = 64;   // rows per wave of pairs_snp_kernel (DESIGN.md 4.12 has both heights measured)

// what both entries refuse before anything is launched
int pairs_check(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim)
{
  if (c->acgt) return fail(c, UVAIA_GPU_ESTATE, "pair counters are taken over the four IUPAC planes: use a default-mode context");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard holds its own pieces only: pairs are counted in a plain context");
  if (row0 > c->db_n || n_rows > c->db_n - row0) return fail(c, UVAIA_GPU_EINVAL, "rows %zu..%zu lie outside the database of %zu references", row0, row0 + n_rows, c->db_n);
  if (col0 > c->db_n || n_cols > c->db_n - col0) return fail(c, UVAIA_GPU_EINVAL, "columns %zu..%zu lie outside the database of %zu references", col0, col0 + n_cols, c->db_n);
  if (trim > (size_t)c->nchar || 2 * trim > (size_t)c->nchar) return fail(c, UVAIA_GPU_EINVAL, "trim %zu on both sides leaves nothing of %d sites", trim, c->nchar);
  return 0;
}

// nothing of this context may still be reading or writing the resident planes (searches in flight, a rebuild of the derived planes shares the streams)
int pairs_wait(uvaia_gpu_ctx *c)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = settle_derive(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return sync_scan_streams(c);
}

int pairs_add_ms(uvaia_gpu_ctx *c, int which)
{ // (the stream has been waited for)
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
  c->pairs.ms[which] += ms;
  return 0;
}

// the row operand records of rows [row0, row0 + n) (n <= PAIRS_LAUNCH_ROWS), padded to whole blocks of 64 rows; waits for them (the time is read)
template <int D> int pairs_build_rows(uvaia_gpu_ctx *c, size_t row0, size_t n, size_t trim)
{
  const size_t rows_pad = (n + 63) / 64 * 64;
  if (int rc = c->pairs.d_rec.reserve(c, PAIRS_LAUNCH_ROWS * (size_t)c->W4 * PAIRS_CNT_DW)) return rc;     // one size for both forms: no regrowth between calls
  HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
  hipLaunchKernelGGL((pairs_rows_kernel<D>), dim3((unsigned)(rows_pad / 64), (unsigned)((c->W4 + 3) / 4)), dim3(256), 0, c->st.stream,
                     (const uint4 *)c->db.planes, c->W4, (long long)row0, (int)n, (int)trim, (int)((size_t)c->nchar - trim), c->pairs.d_rec.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return pairs_add_ms(c, 0);
}

inline unsigned pairs_grid(size_t n_rows, int rt, int n_ctiles) { return (unsigned)((n_rows + rt - 1) / rt) * (unsigned)((n_ctiles + 3) / 4); }

// a clustering is open, and over the database as it is now (the forest has one node per reference resident at `begin`)
int link_state(uvaia_gpu_ctx *c)
{
  const auto &k = c->pairs.link;
  if (!k.begun) return fail(c, UVAIA_GPU_ESTATE, "no clustering is open: call uvaia_gpu_db_link_begin first");
  if (k.db_gen != c->db_gen || k.n != c->db_n) return fail(c, UVAIA_GPU_ESTATE, "the database changed since uvaia_gpu_db_link_begin: begin again");
  return 0;
}

}  // namespace

extern "C" {

int uvaia_gpu_db_pairs(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int what, int32_t *out, size_t ld)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (what != UVAIA_GPU_PAIRS_SNP && what != UVAIA_GPU_PAIRS_COUNTS && what != UVAIA_GPU_PAIRS_SNP_ALT) return fail(c, UVAIA_GPU_EINVAL, "unknown kind of pair output %d", what);
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, trim)) return rc;
  if (!n_rows || !n_cols) return 0;
  if (!out || ld < n_cols) return fail(c, UVAIA_GPU_EINVAL, "NULL output or a leading dimension below the %zu columns", n_cols);
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  const bool counts = what == UVAIA_GPU_PAIRS_COUNTS;
  const size_t per = counts ? UVAIA_GPU_PAIR_NCOUNT : 1;
  const int rt = counts ? PAIRS_CNT_RT : what == UVAIA_GPU_PAIRS_SNP ? PAIRS_SNP_RT : PAIRS_SNP_RT_ALT;
  if (int rc = c->pairs.d_out.reserve(c, std::min(n_rows, PAIRS_LAUNCH_ROWS) * std::min(n_cols, PAIRS_LAUNCH_COLS) * per)) return rc;
  const uint4 *db = c->db.planes;
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (int rc = counts ? pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, trim) : pairs_build_rows<PAIRS_SNP_DW>(c, row0 + rb, nr, trim)) return rc;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + rt - 1) / rt);
      const dim3 grid(pairs_grid(nr, rt, n_ct));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      if (counts)
        hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_DENSE>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct,
                           (long long)c0, (int)nc, c->pairs.d_out.p, nc, 0, 0, 0, (uvaia_gpu_pair *)nullptr, 0ull, (unsigned long long *)nullptr, 0, (uint32_t *)nullptr);
      else if (rt == 32)
        hipLaunchKernelGGL((pairs_snp_kernel<32>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, c->pairs.d_out.p, nc);
      else
        hipLaunchKernelGGL((pairs_snp_kernel<64>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, c->pairs.d_out.p, nc);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      HIPCHK(c, hipMemcpy2DAsync(out + (rb * ld + cb) * per, ld * per * sizeof(int32_t), c->pairs.d_out.p, nc * per * sizeof(int32_t), nc * per * sizeof(int32_t), nr,
                                 hipMemcpyDeviceToHost, c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));
      if (int rc = pairs_add_ms(c, 1)) return rc;
    }
  }
  return 0;
}

int uvaia_gpu_db_pairs_within(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int metric, int max_dist, int upper,
                              uvaia_gpu_pair *out, size_t cap, unsigned long long *n_found)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (metric != UVAIA_GPU_DIST_SNP && metric != UVAIA_GPU_DIST_UVAIA) return fail(c, UVAIA_GPU_EINVAL, "unknown metric %d", metric);
  if (max_dist < 0) return fail(c, UVAIA_GPU_EINVAL, "negative distance %d", max_dist);
  if (!n_found || (cap && !out)) return fail(c, UVAIA_GPU_EINVAL, "NULL list or count");
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, trim)) return rc;
  *n_found = 0;
  if (!n_rows || !n_cols) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  const size_t launch_pairs = std::min(n_rows, PAIRS_LAUNCH_ROWS) * std::min(n_cols, PAIRS_LAUNCH_COLS);
  if (int rc = c->pairs.d_list.reserve(c, std::max<size_t>(1, std::min(cap, launch_pairs)))) return rc;
  if (int rc = c->pairs.d_count.reserve(c, 1)) return rc;
  const uint4 *db = c->db.planes;
  unsigned long long found = 0;
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (int rc = pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, trim)) return rc;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      if (upper && c0 + nc <= row0 + rb + 1) continue;           // no pair of this launch has row < col
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + PAIRS_CNT_RT - 1) / PAIRS_CNT_RT);
      // what of the caller's list is still free bounds the stores of this launch (never more than the launch has pairs: the device list's size)
      const unsigned long long room = found < cap ? std::min<unsigned long long>(cap - found, nr * nc) : 0ull;
      HIPCHK(c, hipMemsetAsync(c->pairs.d_count.p, 0, sizeof(unsigned long long), c->st.stream));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_LIST>), dim3(pairs_grid(nr, PAIRS_CNT_RT, n_ct)), dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p,
                         (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, (int *)nullptr, (size_t)0, metric, max_dist, upper ? 1 : 0,
                         c->pairs.d_list.p, room, c->pairs.d_count.p, 0, (uint32_t *)nullptr);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      unsigned long long n_here = 0;
      HIPCHK(c, hipMemcpyAsync(&n_here, c->pairs.d_count.p, sizeof n_here, hipMemcpyDeviceToHost, c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));
      if (int rc = pairs_add_ms(c, 2)) return rc;
      const unsigned long long take = std::min(n_here, room);
      if (take) HIPCHK(c, hipMemcpy(out + found, c->pairs.d_list.p, (size_t)take * sizeof(uvaia_gpu_pair), hipMemcpyDeviceToHost));
      found += n_here;
    }
  }
  *n_found = found;
  if (found <= cap && found > 1) {
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(out, out + found, [](const uvaia_gpu_pair &a, const uvaia_gpu_pair &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    c->pairs.ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

void uvaia_gpu_pairs_ms(uvaia_gpu_ctx *c, double out[3], int reset)
{
  if (!c) return;
  if (out) for (int i = 0; i < 3; i++) out[i] = c->pairs.ms[i];
  if (reset) c->pairs.ms[0] = c->pairs.ms[1] = c->pairs.ms[2] = 0.;
}

// ---- single-linkage clusters: the pairs within a distance united in a forest on the device
int uvaia_gpu_db_link_begin(uvaia_gpu_ctx *c, size_t trim, int metric, int max_dist, int min_compared)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (metric != UVAIA_GPU_DIST_SNP && metric != UVAIA_GPU_DIST_UVAIA) return fail(c, UVAIA_GPU_EINVAL, "unknown metric %d", metric);
  if (max_dist < 0) return fail(c, UVAIA_GPU_EINVAL, "negative distance %d", max_dist);
  if (min_compared < 0) return fail(c, UVAIA_GPU_EINVAL, "negative floor of compared sites %d", min_compared);
  if (int rc = pairs_check(c, 0, c->db_n, 0, c->db_n, trim)) return rc;
  if (c->db_n > 0xFFFFFFFFull) return fail(c, UVAIA_GPU_EINVAL, "cluster labels are 32-bit database positions: %zu references are too many", c->db_n);
  auto &k = c->pairs.link;
  k.begun = false;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.d_parent.reserve(c, std::max<size_t>(1, c->db_n))) return rc;
  if (c->db_n) {
    hipLaunchKernelGGL(pairs_link_init_kernel, dim3((unsigned)((c->db_n + 255) / 256)), dim3(256), 0, c->st.stream, c->pairs.d_parent.p, (uint32_t)c->db_n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
  }
  k.begun = true; k.db_gen = c->db_gen; k.n = c->db_n; k.trim = trim; k.metric = metric; k.max_dist = max_dist; k.min_compared = min_compared;
  return 0;
}

int uvaia_gpu_db_link(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, unsigned long long *n_links)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = link_state(c)) return rc;
  if (!n_links) return fail(c, UVAIA_GPU_EINVAL, "NULL count of links");
  const auto &k = c->pairs.link;
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, k.trim)) return rc;
  if (!n_rows || !n_cols) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  if (int rc = c->pairs.d_count.reserve(c, 1)) return rc;
  const bool snp = k.metric == UVAIA_GPU_DIST_SNP;
  const int rt = snp ? PAIRS_SNP_RT : PAIRS_CNT_RT;
  const uint4 *db = c->db.planes;
  const uint32_t *rec = nullptr;
  HIPCHK(c, hipMemsetAsync(c->pairs.d_count.p, 0, sizeof(unsigned long long), c->st.stream));      // one count for the launches of this call
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (col0 + n_cols <= row0 + rb + 1) break;                   // this band and every later one lie at or below the diagonal
    if (int rc = snp ? pairs_build_rows<PAIRS_SNP_DW>(c, row0 + rb, nr, k.trim) : pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, k.trim)) return rc;
    rec = c->pairs.d_rec.p;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      if (c0 + nc <= row0 + rb + 1) continue;                    // no pair of this launch has row < col
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + rt - 1) / rt);
      const dim3 grid(pairs_grid(nr, rt, n_ct));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      if (!snp)
        hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_LINK>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           (int *)nullptr, (size_t)0, k.metric, k.max_dist, 1, (uvaia_gpu_pair *)nullptr, 0ull, c->pairs.d_count.p, k.min_compared, c->pairs.d_parent.p);
      else if (k.min_compared > 0)
        hipLaunchKernelGGL((pairs_link_snp_kernel<true>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           k.max_dist, k.min_compared, c->pairs.d_parent.p, c->pairs.d_count.p);
      else
        hipLaunchKernelGGL((pairs_link_snp_kernel<false>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           k.max_dist, 0, c->pairs.d_parent.p, c->pairs.d_count.p);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));             // (the next band's row records overwrite the ones this launch reads)
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
      c->pairs.link_ms += ms;
    }
  }
  unsigned long long found = 0;                                  // read in stream order: behind the memset also where every launch was skipped
  HIPCHK(c, hipMemcpyAsync(&found, c->pairs.d_count.p, sizeof found, hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  *n_links += found;
  return 0;
}

int uvaia_gpu_db_link_labels(uvaia_gpu_ctx *c, uint32_t *labels)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = link_state(c)) return rc;
  const size_t n = c->pairs.link.n;
  if (!n) return 0;
  if (!labels) return fail(c, UVAIA_GPU_EINVAL, "NULL labels");
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  if (int rc = c->pairs.d_labels.reserve(c, n)) return rc;
  HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
  hipLaunchKernelGGL(pairs_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->st.stream, (const uint32_t *)c->pairs.d_parent.p, (uint32_t)n, c->pairs.d_labels.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
  HIPCHK(c, hipMemcpyAsync(labels, c->pairs.d_labels.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
  c->pairs.link_ms += ms;
  return 0;
}

void uvaia_gpu_link_ms(uvaia_gpu_ctx *c, double *ms, int reset)
{
  if (!c) return;
  if (ms) *ms = c->pairs.link_ms;
  if (reset) c->pairs.link_ms = 0.;
}

}  // extern "C"
