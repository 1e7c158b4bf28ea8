// host_qprep.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the query-side tables of the scans
// built on the device (kernels_qprep.inc).  The raw query rows cross PCIe once, through the two pinned staging buffers the reference
// rows use; everything else -- plane words, recoded planes, column classes, rare columns, compressed planes, the kind of every
// (query, word group), the item streams -- is made from them by kernels.  The host only sizes things: it reads back the column
// classes (4 KB per 1 000 columns) to count the polymorphic and rare columns and list them in compressed order, and the record lengths
// of the item streams (one int per super-tile and group) to place the records and cut each stream into the waves' shares.
// Same bytes as build_query_tables_host (host_qtables.inc): tests/test_query_prep_gpu.py compares every table.
namespace {

template <typename T>
int qprep_alloc(DevBuf<T> &b, size_t n_elems, bool zero, hipStream_t s)
{
  n_elems = std::max<size_t>(n_elems, 1);
  if (int rc = b.reserve(nullptr, n_elems)) return rc;
  if (zero) HIPCHK((uvaia_gpu_ctx *)nullptr, hipMemsetAsync(b, 0, n_elems * sizeof(T), s));
  return 0;
}

int build_query_tables_device(uvaia_gpu_ctx *c, const uvaia_gpu_query *q, const uvaia_gpu_tuning &tn, int lo, int hi)
{
#define OPENCHK(call) HIP_TRY(call, return fail(nullptr, code_, "%s failed: %s", #call, hipGetErrorString(e_)))      /* the caller closes the half-made context */
#define QALLOC(buf, n, zero) do { const int rc_ = qprep_alloc((buf), (n), (zero), s); if (rc_) return rc_; } while (0)      /* the tables, and the work space that goes with this frame */
  hipStream_t s = c->st.stream;
  const int Wp = c->W4 * 4, nq = c->nq;
  const size_t row_words = (size_t)Wp * c->NQ;

  // ---- query rows -> plane words
  QALLOC(c->tab.d_qp, (size_t)c->nq_pad * row_words, true);
  c->tab.qtab[0] = {c->tab.d_qp, (size_t)c->nq_pad * row_words * 4};
  DevBuf<unsigned long long> d_bad;
  QALLOC(d_bad, 1, false);
  OPENCHK(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), s));
  for (int done = 0, k = 0; done < nq; done += PACK_CHUNK, k ^= 1) {
    const int m = std::min(PACK_CHUNK, nq - done);
    if (c->stage_busy[k]) { OPENCHK(hipEventSynchronize(c->stage_free[k])); c->stage_busy[k] = false; }
    uint8_t *hs = c->h_stage + (size_t)k * PACK_CHUNK * c->pitch, *ds = c->d_stage + (size_t)k * PACK_CHUNK * c->pitch;
    parallel_for(m, [&](int i) { memcpy(hs + (size_t)i * c->pitch, q->seq[done + i], (size_t)c->nchar); });
    OPENCHK(hipMemcpyAsync(ds, hs, (size_t)m * c->pitch, hipMemcpyHostToDevice, s));
    dim3 grid((unsigned)m, (unsigned)((Wp + 127) / 128));
    if (c->acgt) hipLaunchKernelGGL((qprep_pack_rows_kernel<true>), grid, dim3(128), 0, s, ds, c->pitch, m, done, c->nchar, lo, hi, c->tab.d_pmask, Wp, c->tab.d_qp, d_bad);
    else         hipLaunchKernelGGL((qprep_pack_rows_kernel<false>), grid, dim3(128), 0, s, ds, c->pitch, m, done, c->nchar, lo, hi, c->tab.d_pmask, Wp, c->tab.d_qp, d_bad);
    OPENCHK(hipGetLastError());
    OPENCHK(hipEventRecord(c->stage_free[k], s)); c->stage_busy[k] = true;
  }
  // ---- recoded planes and ambiguity-word lists of the two-counter path
  QALLOC(c->tab.d_amb_q, (size_t)nq * AMB_STRIDE, true);
  c->tab.qtab[2] = {c->tab.d_amb_q, (size_t)nq * AMB_STRIDE * sizeof(int)};
  if (!c->acgt) {
    QALLOC(c->tab.d_qp2, (size_t)c->nq_pad * Wp * 4, true);
    c->tab.qtab[1] = {c->tab.d_qp2, (size_t)c->nq_pad * Wp * 4 * 4};
    hipLaunchKernelGGL(qprep_recode_kernel, dim3((unsigned)nq), dim3(64), 0, s, c->tab.d_qp, Wp, c->tab.d_qp2, c->tab.d_amb_q);
    OPENCHK(hipGetLastError());
  }
  // ---- column classes, rare columns
  const int n_shares = std::max(1, std::min(64, nq / 32)), per_share = (nq + n_shares - 1) / n_shares;
  DevBuf<uint32_t> d_acc; DevBuf<int> d_cnt;
  QALLOC(d_acc, (size_t)Wp * 5, true);
  QALLOC(c->tab.d_cls, (size_t)Wp * 4, true);
  QALLOC(c->tab.d_rmask, (size_t)Wp, true);
  c->tab.qtab[3] = {c->tab.d_cls, (size_t)Wp * 4 * 4}; c->tab.qtab[4] = {c->tab.d_rmask, (size_t)Wp * 4};
  {
    dim3 grid((unsigned)((Wp + 63) / 64), (unsigned)n_shares);
    if (c->acgt) hipLaunchKernelGGL((qprep_classes_kernel<true>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, per_share, d_acc);
    else         hipLaunchKernelGGL((qprep_classes_kernel<false>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, per_share, d_acc);
    hipLaunchKernelGGL(qprep_classes_finish_kernel, dim3((unsigned)((Wp + 63) / 64)), dim3(64), 0, s, d_acc, Wp, c->tab.d_cls);
    OPENCHK(hipGetLastError());
  }
  c->tab.rare_max = tn.rare_max > 0 ? tn.rare_max : tn.rare_max < 0 ? 0 : (nq < 64 ? 0 : std::min(64, std::max(4, nq / 64)));
  if (c->fullscan || c->scan_variant != 2) c->tab.rare_max = 0;
  if (c->tab.rare_max > 0) {
    QALLOC(d_cnt, (size_t)Wp * 32 * 4, true);
    dim3 grid((unsigned)((Wp * 32 + 63) / 64), (unsigned)n_shares);
    if (c->acgt) hipLaunchKernelGGL((qprep_rare_count_kernel<true>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, per_share, c->tab.d_cls, d_cnt);
    else         hipLaunchKernelGGL((qprep_rare_count_kernel<false>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, per_share, c->tab.d_cls, d_cnt);
    hipLaunchKernelGGL(qprep_rare_finish_kernel, dim3((unsigned)((Wp * 32 + 63) / 64)), dim3(64), 0, s, d_cnt, Wp, c->tab.rare_max, c->tab.d_cls, c->tab.d_rmask);
    OPENCHK(hipGetLastError());
  }
  // ---- the host sizes the compressed tables: classes back, columns in compressed order out
  std::vector<uint32_t> cls((size_t)Wp * 4), rmask((size_t)Wp);
  unsigned long long bad = ~0ull;
  OPENCHK(hipMemcpyAsync(cls.data(), c->tab.d_cls, cls.size() * 4, hipMemcpyDeviceToHost, s));
  OPENCHK(hipMemcpyAsync(rmask.data(), c->tab.d_rmask, rmask.size() * 4, hipMemcpyDeviceToHost, s));
  OPENCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
  OPENCHK(hipStreamSynchronize(s));
  c->stage_busy[0] = c->stage_busy[1] = false;
  if (bad != ~0ull) return fail(nullptr, UVAIA_GPU_EALPHABET, "query %d holds byte 0x%02x outside the supported alphabet", (int)(bad >> 40), (unsigned)(bad & 0xFFu));
  std::vector<int> cols_p, cols_r;
  for (int w = 0; w < Wp; w++) {
    for (uint32_t m = cls[(size_t)w * 4 + 3]; m; m &= m - 1) cols_p.push_back(w * 32 + __builtin_ctz(m));
    for (uint32_t m = rmask[(size_t)w]; m; m &= m - 1) cols_r.push_back(w * 32 + __builtin_ctz(m));
  }
  c->tab.NP = (int)cols_p.size(); c->tab.NR = (int)cols_r.size();
  c->tab.NP4 = ((c->tab.NP + 31) / 32 + 3) / 4;
  c->tab.NR4 = ((c->tab.NR + 31) / 32 + 3) / 4;
  // (what the polymorphic and the rare columns can take away has to fit the scan's 16-bit deficits: see host_qtables.inc)
  if (c->scan_variant == 2 && (size_t)c->tab.NP4 * 128 + (size_t)c->tab.NR4 * 128 > SCAN3_BIAS - 256) c->scan_variant = 0;
  {   // derive_all_kernel: word groups per wave and the bit positions its gathered columns start at
    int split[DERIVE_SPLIT_INTS];
    build_derive_split(cls.data(), rmask.data(), c->W4, split);
    QALLOC(c->tab.d_split, DERIVE_SPLIT_INTS, false);
    OPENCHK(hipMemcpyAsync(c->tab.d_split, split, sizeof split, hipMemcpyHostToDevice, s));
    OPENCHK(hipStreamSynchronize(s));                         // (split lives on this frame)
    c->tab.qtab[9] = {c->tab.d_split, sizeof split};
  }
  const size_t prow = (size_t)std::max(c->tab.NP4, 1) * 16;
  QALLOC(c->tab.d_qpl, (size_t)c->nq_pad * prow, true);
  QALLOC(c->tab.d_qrare, (size_t)nq * std::max(c->tab.NR4, 1) * 12, true);
  c->tab.qtab[5] = {c->tab.d_qpl, (size_t)c->nq_pad * prow * 4}; c->tab.qtab[6] = {c->tab.d_qrare, (size_t)nq * std::max(c->tab.NR4, 1) * 12 * 4};
  DevBuf<int> d_cols; DevBuf<uint32_t> d_qmin;
  QALLOC(d_cols, cols_p.size() + cols_r.size(), false);
  QALLOC(d_qmin, (size_t)nq * std::max(c->tab.NR4, 1) * 12, true);
  if (!cols_p.empty()) OPENCHK(hipMemcpyAsync(d_cols, cols_p.data(), cols_p.size() * sizeof(int), hipMemcpyHostToDevice, s));
  if (!cols_r.empty()) OPENCHK(hipMemcpyAsync(d_cols + cols_p.size(), cols_r.data(), cols_r.size() * sizeof(int), hipMemcpyHostToDevice, s));
  if (c->tab.NP4 > 0) {
    dim3 grid((unsigned)nq, (unsigned)((c->tab.NP4 * 4 + 63) / 64));
    if (c->acgt) hipLaunchKernelGGL((qprep_compress_kernel<true, false>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, d_cols, c->tab.NP, c->tab.NP4 * 4, c->tab.d_cls, c->tab.d_qpl, prow, (uint32_t *)nullptr);
    else         hipLaunchKernelGGL((qprep_compress_kernel<false, false>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, d_cols, c->tab.NP, c->tab.NP4 * 4, c->tab.d_cls, c->tab.d_qpl, prow, (uint32_t *)nullptr);
    OPENCHK(hipGetLastError());
  }
  if (c->tab.NR4 > 0) {
    dim3 grid((unsigned)nq, (unsigned)((c->tab.NR4 * 4 + 63) / 64));
    if (c->acgt) hipLaunchKernelGGL((qprep_compress_kernel<true, true>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, d_cols + cols_p.size(), c->tab.NR, c->tab.NR4 * 4, c->tab.d_cls, c->tab.d_qrare, (size_t)0, d_qmin);
    else         hipLaunchKernelGGL((qprep_compress_kernel<false, true>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, d_cols + cols_p.size(), c->tab.NR, c->tab.NR4 * 4, c->tab.d_cls, c->tab.d_qrare, (size_t)0, d_qmin);
    OPENCHK(hipGetLastError());
  }
  // ---- the kind of every (query, word group), the sizes of the item-stream records
  const int NWs = c->scan_NW, QS = 64, n_st = c->nq_pad / QS, NX = c->W4 + c->tab.NR4;
  const uint32_t row_b = 256u * (uint32_t)c->scan_R;         // bytes of a query's counter row in a wave's LDS block: 64 lanes x R tiles x 4
  DevBuf<uint8_t> d_kind; DevBuf<int> d_need, d_len, d_cost;
  QALLOC(d_kind, (size_t)nq * c->W4, false);
  QALLOC(d_need, (size_t)c->W4, true);
  QALLOC(d_len, (size_t)n_st * NX, false);
  QALLOC(d_cost, (size_t)n_st * NX, false);
  {
    dim3 grid((unsigned)nq, (unsigned)((c->W4 + 63) / 64));
    if (c->acgt) hipLaunchKernelGGL((qprep_kinds_kernel<true>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, c->tab.d_cls, d_kind, d_need);
    else         hipLaunchKernelGGL((qprep_kinds_kernel<false>), grid, dim3(64), 0, s, c->tab.d_qp, nq, Wp, c->tab.d_cls, d_kind, d_need);
    hipLaunchKernelGGL(qprep_stream_sizes_kernel, dim3((unsigned)NX, (unsigned)n_st), dim3(64), 0, s, d_kind, d_qmin, nq, c->W4, c->tab.NR4, d_len, d_cost);
    OPENCHK(hipGetLastError());
  }
  std::vector<int> need((size_t)c->W4), len((size_t)n_st * NX), cost((size_t)n_st * NX);
  OPENCHK(hipMemcpyAsync(need.data(), d_need, need.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  OPENCHK(hipMemcpyAsync(len.data(), d_len, len.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  OPENCHK(hipMemcpyAsync(cost.data(), d_cost, cost.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  OPENCHK(hipStreamSynchronize(s));
  for (int g = 0; g < c->W4; g++) { c->tab.need_e_groups += (need[(size_t)g] & 1) != 0; c->tab.need_v_groups += (need[(size_t)g] & 2) != 0; c->tab.need_g_groups += (need[(size_t)g] & 4) != 0; }
  // Next to a running scan a replay block with the 22 KB query row fits once per CU, without it seven times (host_qtables.inc)
  if (c->replay_lq < 0) c->replay_lq = (nq < 256) ? 1 : 0;
  // ---- the records' places, each stream cut into NW contiguous shares of about the same cost (two directories: group records, rare records)
  std::vector<long long> at((size_t)n_st * (NX + 1), 0);
  std::vector<uint32_t> sdir((size_t)n_st * 4 * NWs, 0u);
  std::vector<uint8_t> rare_group_used((size_t)std::max(c->tab.NR4, 1), 0);
  size_t total = 0;
  struct Rec { size_t at; uint32_t cost; };
  auto shares = [NWs](const std::vector<Rec> &r, size_t base, size_t end_at, uint32_t *dir) {
    uint64_t tot = 0;
    for (const Rec &x : r) tot += x.cost;
    size_t i = 0; uint64_t done = 0;
    for (int w = 0; w < NWs; w++) {
      const size_t i0 = i;
      const uint64_t goal = tot * (uint64_t)(w + 1) / (uint64_t)NWs;
      while (i < r.size() && (w == NWs - 1 || done + r[i].cost / 2 < goal)) { done += r[i].cost; i++; }
      dir[2 * w] = (uint32_t)(base + (i0 < r.size() ? r[i0].at : end_at));
      dir[2 * w + 1] = (uint32_t)(i - i0);
    }
  };
  for (int st = 0; st < n_st; st++) {
    const size_t base = total;
    size_t pos = 0;
    std::vector<Rec> rec, rare;
    for (int x = 0; x < c->W4; x++) { const int L = len[(size_t)st * NX + x]; if (!L) continue; at[(size_t)st * (NX + 1) + x] = (long long)(base + pos); rec.push_back({pos, (uint32_t)cost[(size_t)st * NX + x]}); pos += (size_t)L; }
    const size_t groups_end = pos;
    at[(size_t)st * (NX + 1) + NX] = (long long)(base + pos); pos += 8;
    for (int x = c->W4; x < NX; x++) { const int L = len[(size_t)st * NX + x]; if (!L) continue; at[(size_t)st * (NX + 1) + x] = (long long)(base + pos); rare.push_back({pos, (uint32_t)cost[(size_t)st * NX + x]}); pos += (size_t)L; rare_group_used[(size_t)(x - c->W4)] = 1; }
    // a wave without records still looks at two headers: it is pointed at the zero headers that end the group records
    shares(rec, base, groups_end, &sdir[(size_t)st * 4 * NWs]);
    shares(rare, base, pos - 8, &sdir[(size_t)st * 4 * NWs + 2 * NWs]);
    total += pos;
  }
  for (uint8_t u : rare_group_used) c->tab.need_r_groups += u;
  if (total + 64 > 0xFFFFFFFFull) return fail(nullptr, UVAIA_GPU_EINVAL, "item streams of %zu dwords", total);
  DevBuf<long long> d_at;
  QALLOC(d_at, at.size(), false);
  QALLOC(c->tab.d_stream, total + 64, true);                     // the kernel prefetches items and headers past the end
  QALLOC(c->tab.d_sdir, sdir.size(), false);
  c->tab.qtab[7] = {c->tab.d_stream, (total + 64) * 4}; c->tab.qtab[8] = {c->tab.d_sdir, sdir.size() * 4};
  OPENCHK(hipMemcpyAsync(d_at, at.data(), at.size() * sizeof(long long), hipMemcpyHostToDevice, s));
  OPENCHK(hipMemcpyAsync(c->tab.d_sdir, sdir.data(), sdir.size() * 4, hipMemcpyHostToDevice, s));
  {
    dim3 grid((unsigned)(NX + 1), (unsigned)n_st);
    if (c->acgt) hipLaunchKernelGGL((qprep_stream_fill_kernel<true>), grid, dim3(64), 0, s, c->tab.d_qp, d_kind, d_qmin, c->tab.d_cls, nq, Wp, c->tab.NP4, c->tab.NR4, d_len, d_at, row_b, c->tab.d_stream);
    else         hipLaunchKernelGGL((qprep_stream_fill_kernel<false>), grid, dim3(64), 0, s, c->tab.d_qp, d_kind, d_qmin, c->tab.d_cls, nq, Wp, c->tab.NP4, c->tab.NR4, d_len, d_at, row_b, c->tab.d_stream);
    OPENCHK(hipGetLastError());
  }
  OPENCHK(hipStreamSynchronize(s));                           // at, sdir live on this frame; the work space goes with it
  return 0;
#undef QALLOC
#undef OPENCHK
}

}  // namespace
