// host_text.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the text row store (include/uvaia_gpu.h, "text
// row store").  Rows that reach the resident database from device memory (uvaia_gpu_db_append_device) leave no text behind on the host, and
// an --acgt context keeps no four-plane image of them either: a command that has to write out the references that entered a heap keeps
// their text here, as text.  Both directions are rows_gather_kernel (kernels_rows.inc): by index, from any alignment, into rows of a
// multiple of 16 bytes.

namespace {

inline size_t text_pitch(const uvaia_gpu_ctx *c) { return ((size_t)c->nchar + 15) / 16 * 16; }

// room for n_rows rows in all; what the store holds is kept
int text_make_room(uvaia_gpu_ctx *c, size_t n_rows)
{
  uvaia_gpu_ctx::Text &t = c->text;
  if (n_rows <= t.cap) return 0;
  const size_t tp = text_pitch(c);
  if (int rc = t.d_store.grow_keeping(c, n_rows * tp, t.n * tp, c->st.stream)) return rc;
  t.cap = n_rows;
  return 0;
}

}  // namespace

extern "C" {

int uvaia_gpu_text_reserve(uvaia_gpu_ctx *c, size_t n_rows)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps no text row store");
  HIPCHK(c, hipSetDevice(c->device));
  return text_make_room(c, n_rows);
}

size_t uvaia_gpu_text_size(const uvaia_gpu_ctx *c) { return c ? c->text.n : 0; }

int uvaia_gpu_text_clear(uvaia_gpu_ctx *c)
{
  if (!c) return UVAIA_GPU_EINVAL;
  c->text.n = 0;
  return 0;
}

int uvaia_gpu_text_append_device(uvaia_gpu_ctx *c, const void *d_rows, size_t pitch, const int *row_index, int n_sel)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (n_sel < 0) return fail(c, UVAIA_GPU_EINVAL, "negative count");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard keeps no text row store");
  if (n_sel == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  long long last = -1;
  if (int rc = rows_last_selected(c, row_index, n_sel, &last)) return rc;
  if (int rc = rows_check_block(c, d_rows, pitch, last)) return rc;
  uvaia_gpu_ctx::Text &t = c->text;
  if (t.n + (size_t)n_sel > t.cap) { if (int rc = text_make_room(c, std::max(t.n + (size_t)n_sel, 2 * t.cap))) return rc; }     // (grows by doubling)
  if (row_index) { if (int rc = rows_upload_selection(c, row_index, n_sel)) return rc; }
  for (int i = 0; i < 2; i++) if (int rc = t.ev[i].make(c)) return rc;
  const size_t tp = text_pitch(c);
  HIPCHK(c, hipEventRecord(t.ev[0], c->st.stream));
  hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)n_sel), dim3(ROWS_TPB), 0, c->st.stream, reinterpret_cast<const uint8_t *>(d_rows), pitch, c->nchar,
                     row_index ? c->rows.d_sel : (const int *)nullptr, 0, t.d_store + t.n * tp, tp);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(t.ev[1], c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));          // the caller may overwrite its rows
  float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, t.ev[0], t.ev[1])); t.ms[0] += ms;
  t.n += (size_t)n_sel;
  return 0;
}

int uvaia_gpu_text_rows(uvaia_gpu_ctx *c, const int *index, int n, char *rows, size_t pitch)
{
  if (!c) return UVAIA_GPU_EINVAL;
  uvaia_gpu_ctx::Text &t = c->text;
  if (n < 0 || (n > 0 && (!index || !rows))) return fail(c, UVAIA_GPU_EINVAL, "bad selection");
  if (pitch < (size_t)c->nchar) return fail(c, UVAIA_GPU_EINVAL, "pitch %zu is below the %d sites of a row", pitch, c->nchar);
  for (int k = 0; k < n; k++)
    if (index[k] < 0 || (size_t)index[k] >= t.n) return fail(c, UVAIA_GPU_EINVAL, "index[%d] = %d lies outside the %zu rows of the text row store", k, index[k], t.n);
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t tp = text_pitch(c);
  const size_t chunk = std::min((size_t)n, c->pool_pad);    // a selection may repeat rows: longer ones go in rounds of a pool
  if (int rc = t.d_out.reserve(c, chunk * tp)) return rc;
  if (int rc = t.d_idx.reserve(c, chunk)) return rc;
  for (int i = 2; i < 4; i++) if (int rc = t.ev[i].make(c)) return rc;
  for (size_t a = 0; a < (size_t)n; a += chunk) {
    const size_t m = std::min(chunk, (size_t)n - a);
    HIPCHK(c, hipMemcpyAsync(t.d_idx, index + a, m * sizeof(int), hipMemcpyHostToDevice, c->st.stream));
    HIPCHK(c, hipEventRecord(t.ev[2], c->st.stream));
    hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)m), dim3(ROWS_TPB), 0, c->st.stream, (const uint8_t *)t.d_store, tp, c->nchar, (const int *)t.d_idx, 0, t.d_out.p, tp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t.ev[3], c->st.stream));
    // one copy for all rows of the round (as unpack_rows_from): straight when the caller's rows have the store's pitch, strided otherwise
    if (pitch == tp) HIPCHK(c, hipMemcpyAsync(rows + a * pitch, t.d_out, m * tp, hipMemcpyDeviceToHost, c->st.stream));
    else HIPCHK(c, hipMemcpy2DAsync(rows + a * pitch, pitch, t.d_out, tp, (size_t)c->nchar, m, hipMemcpyDeviceToHost, c->st.stream));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, t.ev[2], t.ev[3])); t.ms[1] += ms;
  }
  return 0;
}

void uvaia_gpu_text_ms(uvaia_gpu_ctx *c, double out[2], int reset)
{
  if (!c) return;
  if (out) { out[0] = c->text.ms[0]; out[1] = c->text.ms[1]; }
  if (reset) c->text.ms[0] = c->text.ms[1] = 0.;
}

}  // extern "C"
