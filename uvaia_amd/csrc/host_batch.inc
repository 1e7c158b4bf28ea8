// host_batch.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): streamed batches (uvaia_gpu_push, uvaia_gpu_drain) and query preprocessing (pair test, column walk).

extern "C" {

int uvaia_gpu_agree_on_polymorphic(uvaia_gpu_ctx *c, const char *const *seq, int n_seq, uint8_t *out)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_seq < 0 || (n_seq > 0 && (!seq || !out))) return fail(c, UVAIA_GPU_EINVAL, "bad batch");
  if ((size_t)n_seq > c->max_pool) return fail(c, UVAIA_GPU_ESTATE, "batch of %d exceeds max_pool %zu", n_seq, c->max_pool);
  if (n_seq == 0) return 0;
  int rc = ensure_batch_buffers(c); if (rc) return rc;
  rc = pack_rows(c, seq, nullptr, 0, nullptr, n_seq, c->batch, 0);
  if (rc) return rc;
  const int n_tiles = (n_seq + 63) / 64, ppad = n_tiles * 64;
  rc = ensure_cnt4(c, (size_t)c->nq_pad * c->pool_pad); if (rc) return rc;
  const bool prof = c->stats.profile; c->stats.profile = false;     // not the nearest-neighbour scan the statistics describe
  rc = ensure_qpoly(c); if (rc) return rc;
  rc = launch_scan(c, c->batch, 0, n_tiles, c->tab.d_qpoly, c->nq, c->state.d_cnt, ppad, 0.0);
  c->stats.profile = prof;
  if (rc) return rc;
  DevBuf<uint8_t> d_out;
  const size_t bytes = (size_t)n_seq * c->nq;
  if (int rc_ = d_out.reserve(c, bytes)) return rc_;
  dim3 grid((n_seq + 255) / 256, c->nq);
  if (c->acgt) hipLaunchKernelGGL((agree_kernel<true>), grid, dim3(256), 0, c->st.stream, c->state.d_cnt, ppad, c->nq, n_seq, d_out);
  else         hipLaunchKernelGGL((agree_kernel<false>), grid, dim3(256), 0, c->st.stream, c->state.d_cnt, ppad, c->nq, n_seq, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->st.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st.stream);
  if (e != hipSuccess) return fail(c, UVAIA_GPU_EHIP, "agree_on_polymorphic: %s", hipGetErrorString(e));
  return 0;
}

// create_query_indices (src/fastaseq.c:732-777) needs no context: the query rows go to the device in batches through a pinned
// staging buffer (host copies threaded), two small kernels per batch, the per-column result comes back as two byte arrays.
int uvaia_gpu_query_columns(const char *const *seq, int n_query, int nchar, size_t trim, int acgt, int device, char *consensus, unsigned char *some_missing)
{
  if (!seq || !consensus || !some_missing || n_query < 1 || nchar < 1) return fail(nullptr, UVAIA_GPU_EINVAL, "empty query set");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, UVAIA_GPU_ENODEV, "no HIP device available: the MI355X engine has no CPU fallback");
  int caller_device = -1;
  if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
  if (device < 0) device = caller_device < 0 ? 0 : caller_device;
  if (device >= ndev || hipSetDevice(device) != hipSuccess) return fail(nullptr, UVAIA_GPU_ENODEV, "device %d is not usable", device);
  struct RestoreDevice { int d; ~RestoreDevice() { if (d >= 0) hipSetDevice(d); } } restore_{caller_device};   // no context: the caller's current device is left as it was
  const int lo = (int)std::min<size_t>(trim, (size_t)nchar), hi = std::max(lo, nchar - (int)std::min<size_t>(trim, (size_t)nchar));
  memset(consensus, 'N', (size_t)nchar);
  memset(some_missing, 0, (size_t)nchar);
  if (hi <= lo) return 0;
  const size_t pitch = ((size_t)nchar + 63) / 64 * 64;
  const int batch = (int)std::max<size_t>(64, std::min<size_t>(4096, ((size_t)96 << 20) / pitch) / 64 * 64);      // rows per batch: at most 96 MB of staging
  const int groups = batch / 64;
  // no context: what this call makes goes with this frame, last to first -- the wait for the stream, the events and arrays, the stream
  Stream st;
  PinnedBuf h_rows;
  DevBuf<uint8_t> d_rows, d_pf, d_pl, d_first, d_flags;
  Event freed[2];
  struct Wait { const Stream &s; ~Wait() { if (s) hipStreamSynchronize(s); } } wait_{st};
  uvaia_gpu_ctx *const none = nullptr;
#define QCHK(call) HIPCHK(none, call)
  QCHK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  if (int rc = h_rows.alloc(none, (size_t)2 * batch * pitch)) return rc;
  if (int rc = d_rows.reserve(none, (size_t)2 * batch * pitch)) return rc;
  if (int rc = d_pf.reserve(none, (size_t)groups * nchar)) return rc;
  if (int rc = d_pl.reserve(none, (size_t)groups * nchar)) return rc;
  if (int rc = d_first.reserve(none, (size_t)nchar)) return rc;
  if (int rc = d_flags.reserve(none, (size_t)nchar)) return rc;
  QCHK(hipMemsetAsync(d_first, 'N', (size_t)nchar, st)); QCHK(hipMemsetAsync(d_flags, 0, (size_t)nchar, st));
  for (Event &e : freed) if (int rc = e.make(none, hipEventDisableTiming)) return rc;
  const unsigned gx = (unsigned)((hi - lo + 255) / 256);
  int k = 0;
  for (int a = 0; a < n_query; a += batch, k++) {
    const int m = std::min(batch, n_query - a), b = k & 1;
    if (k >= 2) QCHK(hipEventSynchronize(freed[b]));                 // the staging half's previous batch has been consumed
    uint8_t *hb = h_rows + (size_t)b * batch * pitch, *db = d_rows + (size_t)b * batch * pitch;
    for (int i = 0; i < m; i++) if (!seq[a + i]) return fail(nullptr, UVAIA_GPU_EINVAL, "query %d is NULL", a + i);
    parallel_for(m, [&](int i) { memcpy(hb + (size_t)i * pitch, seq[a + i], (size_t)nchar); });
    QCHK(hipMemcpyAsync(db, hb, (size_t)m * pitch, hipMemcpyHostToDevice, st));
    const int ng = (m + 63) / 64;
    hipLaunchKernelGGL(query_columns_partial_kernel, dim3(gx, (unsigned)ng), dim3(256), 0, st, db, pitch, m, lo, hi, acgt ? 1 : 0, d_pf, d_pl, nchar);
    hipLaunchKernelGGL(query_columns_merge_kernel, dim3(gx), dim3(256), 0, st, d_pf, d_pl, ng, lo, hi, nchar, d_first, d_flags);
    QCHK(hipGetLastError());
    QCHK(hipEventRecord(freed[b], st));
  }
  std::vector<uint8_t> first((size_t)nchar), flags((size_t)nchar);
  QCHK(hipMemcpyAsync(first.data(), d_first, (size_t)nchar, hipMemcpyDeviceToHost, st));
  QCHK(hipMemcpyAsync(flags.data(), d_flags, (size_t)nchar, hipMemcpyDeviceToHost, st));
  QCHK(hipStreamSynchronize(st));
#undef QCHK
  for (int c = lo; c < hi; c++) {
    consensus[c] = (flags[(size_t)c] & 1) ? '#' : (char)first[(size_t)c];
    some_missing[c] = (flags[(size_t)c] & 2) ? 1 : 0;
  }
  return 0;
}

int uvaia_gpu_push(uvaia_gpu_ctx *c, const char *const *seq, const int *non_n, int n_ref, int64_t ordinal0, uint8_t *entered)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_ref < 0 || (n_ref > 0 && !seq)) return fail(c, UVAIA_GPU_EINVAL, "bad batch");
  if ((size_t)n_ref > c->max_pool) return fail(c, UVAIA_GPU_ESTATE, "batch of %d exceeds max_pool %zu", n_ref, c->max_pool);
  if (c->act_q0 != 0 || c->act_q1 != c->nq) return fail(c, UVAIA_GPU_ESTATE, "streamed batches act on the whole query set: query shards use the resident calls");
  if (n_ref == 0) return 0;
  int rc = ensure_batch_buffers(c); if (rc) return rc;
  rc = pack_rows(c, seq, nullptr, 0, non_n, n_ref, c->batch, 0);
  if (rc) return rc;
  const int n_tiles = (n_ref + 63) / 64;
  HIPCHK(c, hipMemsetAsync(c->state.d_entered, 0, (size_t)n_tiles * 64, c->st.stream));
  rc = run_batch(c, c->batch, 0, n_tiles, 0, n_ref, ordinal0);
  if (rc) return rc;
  if (entered) HIPCHK(c, hipMemcpyAsync(entered, c->state.d_entered, (size_t)n_ref, hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return collect_events(c);
}

int uvaia_gpu_drain(uvaia_gpu_ctx *c, int *n_items, int *max_incompatible, int *scores, int64_t *ordinals)
{
  if (!c || !n_items || !scores || !ordinals) return c ? fail(c, UVAIA_GPU_EINVAL, "NULL output") : UVAIA_GPU_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  planes_idle(c, true, false);
  const size_t ne = (size_t)c->nq * (c->k + 1);
  std::vector<int> h(ne * HEAP_ENTRY), T(c->nq);
  HIPCHK(c, hipMemcpy(h.data(), c->state.d_heap, h.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(n_items, c->state.d_n, (size_t)c->nq * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(T.data(), c->state.d_T, (size_t)c->nq * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < ne; e++) {
    for (int s = 0; s < 6; s++) scores[e * 6 + s] = h[e * HEAP_ENTRY + s];
    ordinals[e] = (int64_t)(((uint64_t)(uint32_t)h[e * HEAP_ENTRY + 7] << 32) | (uint32_t)h[e * HEAP_ENTRY + 6]);
  }
  if (max_incompatible) memcpy(max_incompatible, T.data(), (size_t)c->nq * sizeof(int));
  return collect_events(c);
}


}  // extern "C"
