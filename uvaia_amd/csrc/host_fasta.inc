// host_fasta.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the FASTA parser's handle and its entries
// (include/uvaia_gpu.h, "FASTA text split into rows on the device"; the kernels are in kernels_fasta.inc).

struct uvaia_gpu_fasta {
  int device = 0, max_records = 0;
  size_t block_bytes = 0;
  std::string err;
  Stream st;
  DevBuf<uint8_t> d_text, d_rows;        // the block as handed in (16 bytes of slack on either side); the rows of pass 2
  DevBuf<int4> d_sum;                    // per chunk: summary, then carry
  DevBuf<int> d_hdr;                     // first '>' of max_records + 1 header lines, the starts of those lines, the count of all
  DevBuf<FastaRec> d_rec;                // max_records records and the text before the first header line
  DevBuf<int2> d_body;                   // per row of pass 2 / per selected sequence: offset and length of its body
  DevBuf<int> d_acgt;                    // per record: its A C G T sites
  DevBuf<long long> d_seqoff;            // per selected sequence, and one more: where it begins in d_seq
  DevBuf<uint8_t> d_seq;                 // the selected sequences back to back, FASTA_SEQ_GUARD guard bytes behind them
  std::vector<long long> seqoff;
  std::vector<uint8_t> chosen;           // per record: is it in the selection being checked
  std::vector<uvaia_gpu_fasta_record> rec;
  std::vector<int2> body;
  Event ev[6], ev_seq[4];
  int n_rec = 0, n_bytes = 0, mis = 0, n_rows = 0;   // of the last scan / rows call
  size_t pitch = 0, bad_off = 0;         // what the last scan refused
  unsigned bad_kind = 0;
  double ms[2] = {0., 0.}, ms_seq[2] = {0., 0.};
  long long seq_bytes = -1;              // of the last fasta_sequences since the last scan; -1: there was none
};

constexpr size_t FASTA_SEQ_GUARD = 64;   // bytes behind the sequences that fasta_sequences sets to 0xEE and its kernel leaves alone

static_assert(sizeof(FastaRec) == sizeof(uvaia_gpu_fasta_record) && sizeof(FastaRec) == 32, "the record table is a fixed layout");

namespace {

thread_local std::string g_fasta_open_error;

int fasta_fail(uvaia_gpu_fasta *f, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (f) f->err = buf; else g_fasta_open_error = buf;
  return code;
}

int fasta_open_body(uvaia_gpu_fasta *f)
{
  HIPCHK(f, hipSetDevice(f->device));
  HIPCHK(f, hipStreamCreateWithFlags(&f->st.s, hipStreamNonBlocking));
  for (Event &e : f->ev) if (int rc = e.make(f)) return rc;
  for (Event &e : f->ev_seq) if (int rc = e.make(f)) return rc;
  const size_t cap = (size_t)f->max_records + 1;
  if (int rc = f->d_text.reserve(f, f->block_bytes + 48)) return rc;
  if (int rc = f->d_sum.reserve(f, (f->block_bytes + 16) / FASTA_CHUNK + 2)) return rc;
  if (int rc = f->d_hdr.reserve(f, 2 * cap + 1)) return rc;
  if (int rc = f->d_rec.reserve(f, cap)) return rc;
  return 0;
}

}  // namespace

extern "C" {

int uvaia_gpu_fasta_open(uvaia_gpu_fasta **out, int device, size_t block_bytes, int max_records)
{
  if (!out) return fasta_fail(nullptr, UVAIA_GPU_EINVAL, "NULL handle");
  *out = nullptr;
  if (block_bytes < 1 || block_bytes > ((size_t)1 << 30)) return fasta_fail(nullptr, UVAIA_GPU_EINVAL, "a text block of %zu bytes: 1 byte to 1 GiB", block_bytes);
  if (max_records < 1 || max_records > (1 << 26)) return fasta_fail(nullptr, UVAIA_GPU_EINVAL, "%d records per scan: 1 to %d", max_records, 1 << 26);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return fasta_fail(nullptr, UVAIA_GPU_ENODEV, "no HIP device"); }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return fasta_fail(nullptr, UVAIA_GPU_ENODEV, "no current HIP device"); }
  if (device >= n_dev) return fasta_fail(nullptr, UVAIA_GPU_ENODEV, "device %d of %d", device, n_dev);
  uvaia_gpu_fasta *f = new (std::nothrow) uvaia_gpu_fasta;
  if (!f) return fasta_fail(nullptr, UVAIA_GPU_ENOMEM, "out of host memory");
  f->device = device; f->block_bytes = block_bytes; f->max_records = max_records;
  if (int rc = fasta_open_body(f)) { g_fasta_open_error = f->err; delete f; return rc; }
  *out = f;
  return 0;
}

void uvaia_gpu_fasta_close(uvaia_gpu_fasta *f)
{
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->st.s) (void)hipStreamSynchronize(f->st);
  delete f;
}

const char *uvaia_gpu_fasta_last_error(const uvaia_gpu_fasta *f) { return f ? f->err.c_str() : g_fasta_open_error.c_str(); }

int uvaia_gpu_fasta_scan(uvaia_gpu_fasta *f, const void *text, size_t n_bytes, int final, int *n_records, size_t *consumed)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (!n_records || !consumed || (n_bytes && !text)) return fasta_fail(f, UVAIA_GPU_EINVAL, "bad scan arguments");
  *n_records = 0; *consumed = 0;
  f->n_rec = 0; f->n_rows = 0; f->n_bytes = 0; f->rec.clear(); f->seq_bytes = -1;
  f->bad_kind = 0; f->bad_off = 0;
  if (n_bytes > f->block_bytes) return fasta_fail(f, UVAIA_GPU_EINVAL, "%zu bytes of text, the parser was opened for blocks of %zu", n_bytes, f->block_bytes);
  if (n_bytes == 0) return 0;
  HIPCHK(f, hipSetDevice(f->device));
  const int n = (int)n_bytes, mis = (int)(reinterpret_cast<uintptr_t>(text) & 15), cap = f->max_records + 1;
  const int n_chunks = (int)(((size_t)n + mis + FASTA_CHUNK - 1) / FASTA_CHUNK);
  if ((size_t)n_chunks > f->d_sum.cap) return fasta_fail(f, UVAIA_GPU_EINVAL, "internal: %d chunks", n_chunks);
  // 16 bytes in front of the text stay untouched, the pieces behind it are read up to the next multiple of 16: both inside the buffer
  const uint4 *base = reinterpret_cast<const uint4 *>(f->d_text.p + 16);
  HIPCHK(f, hipMemcpyAsync(f->d_text.p + 16 + mis, text, n_bytes, hipMemcpyHostToDevice, f->st));
  int *hdr_gt = f->d_hdr, *hdr_line = f->d_hdr + cap, *d_total = f->d_hdr + 2 * (size_t)cap;
  HIPCHK(f, hipEventRecord(f->ev[0], f->st));
  hipLaunchKernelGGL(fasta_chunk_summary_kernel, dim3((unsigned)n_chunks), dim3(FASTA_TPB), 0, f->st, base, mis, n, f->d_sum.p);
  hipLaunchKernelGGL(fasta_chunk_scan_kernel, dim3(1), dim3(FASTA_TPB), 0, f->st, f->d_sum.p, n_chunks, d_total);
  hipLaunchKernelGGL(fasta_headers_kernel, dim3((unsigned)n_chunks), dim3(FASTA_TPB), 0, f->st, base, mis, n, (const int4 *)f->d_sum.p, cap, hdr_gt, hdr_line);
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev[1], f->st));
  int total = 0;
  HIPCHK(f, hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  if (total < 0) return fasta_fail(f, UVAIA_GPU_EHIP, "internal: %d header lines", total);
  const int known = std::min(total, cap);
  const int n_rec = total > f->max_records ? f->max_records : (final ? total : std::max(total - 1, 0));
  HIPCHK(f, hipEventRecord(f->ev[2], f->st));
  hipLaunchKernelGGL(fasta_records_kernel, dim3((unsigned)((n_rec + 1 + FASTA_TPB / 64 - 1) / (FASTA_TPB / 64))), dim3(FASTA_TPB), 0, f->st, base, mis, n, n_rec, known, (const int *)hdr_gt, (const int *)hdr_line, f->d_rec.p);
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev[3], f->st));
  f->rec.resize((size_t)n_rec + 1);
  HIPCHK(f, hipMemcpyAsync(f->rec.data(), f->d_rec.p, ((size_t)n_rec + 1) * sizeof(FastaRec), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  for (int i = 0; i < 2; i++) { float ms = 0; HIPCHK(f, hipEventElapsedTime(&ms, f->ev[2 * i], f->ev[2 * i + 1])); f->ms[0] += ms; }
  // irregular input: the text before the first header line, then the records in their order
  const uvaia_gpu_fasta_record pre = f->rec[n_rec];
  f->rec.resize((size_t)n_rec);
  if (pre.flags & UVAIA_GPU_FASTA_NUL) { f->bad_kind = UVAIA_GPU_FASTA_NUL; f->bad_off = pre.bad_off; }
  else if (pre.flags & UVAIA_GPU_FASTA_TEXT) { f->bad_kind = UVAIA_GPU_FASTA_TEXT; f->bad_off = pre.name_off; }
  for (int k = 0; k < n_rec && !f->bad_kind; k++) {
    if (f->rec[k].flags & UVAIA_GPU_FASTA_NUL) { f->bad_kind = UVAIA_GPU_FASTA_NUL; f->bad_off = f->rec[k].bad_off; }
    else if (f->rec[k].flags & UVAIA_GPU_FASTA_EMPTY) { f->bad_kind = UVAIA_GPU_FASTA_EMPTY; f->bad_off = f->rec[k].name_off - 1; }
  }
  if (f->bad_kind) {
    f->rec.clear();
    if (f->bad_kind == UVAIA_GPU_FASTA_NUL) return fasta_fail(f, UVAIA_GPU_EINVAL, "FASTA text: a NUL byte at offset %zu", f->bad_off);
    if (f->bad_kind == UVAIA_GPU_FASTA_TEXT) return fasta_fail(f, UVAIA_GPU_EINVAL, "FASTA text: a line that is not blank before the first header line, at offset %zu", f->bad_off);
    return fasta_fail(f, UVAIA_GPU_EINVAL, "FASTA text: a record without sequence, its header at offset %zu", f->bad_off);
  }
  f->n_rec = n_rec; f->n_bytes = n; f->mis = mis;
  *n_records = n_rec;
  *consumed = n_rec ? (size_t)f->rec[n_rec - 1].body_off + f->rec[n_rec - 1].body_len : (size_t)pre.body_len;
  return 0;
}

unsigned uvaia_gpu_fasta_bad(const uvaia_gpu_fasta *f, size_t *offset)
{
  if (!f) return 0;
  if (offset) *offset = f->bad_off;
  return f->bad_kind;
}

int uvaia_gpu_fasta_records(uvaia_gpu_fasta *f, uvaia_gpu_fasta_record *out)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (f->n_rec && !out) return fasta_fail(f, UVAIA_GPU_EINVAL, "NULL table");
  if (f->n_rec) memcpy(out, f->rec.data(), (size_t)f->n_rec * sizeof(uvaia_gpu_fasta_record));
  return 0;
}

int uvaia_gpu_fasta_rows(uvaia_gpu_fasta *f, int nchar, const void **d_rows, size_t *pitch, int *n_rows, int *row_of_record)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (nchar < 1 || !d_rows || !pitch || !n_rows) return fasta_fail(f, UVAIA_GPU_EINVAL, "bad rows arguments");
  f->body.clear();
  for (int k = 0; k < f->n_rec; k++) {
    const bool mine = f->rec[k].seq_len == (uint32_t)nchar;
    if (row_of_record) row_of_record[k] = mine ? (int)f->body.size() : -1;
    if (mine) f->body.push_back(make_int2((int)f->rec[k].body_off, (int)f->rec[k].body_len));
  }
  f->pitch = ((size_t)nchar + 15) & ~(size_t)15;
  f->n_rows = 0;
  *d_rows = nullptr; *pitch = f->pitch; *n_rows = 0;
  if (f->body.empty()) return 0;
  HIPCHK(f, hipSetDevice(f->device));
  if (int rc = f->d_rows.reserve(f, f->body.size() * f->pitch)) return rc;
  if (int rc = f->d_body.reserve(f, f->body.size())) return rc;
  HIPCHK(f, hipMemcpyAsync(f->d_body.p, f->body.data(), f->body.size() * sizeof(int2), hipMemcpyHostToDevice, f->st));
  HIPCHK(f, hipEventRecord(f->ev[4], f->st));
  hipLaunchKernelGGL(fasta_rows_kernel, dim3((unsigned)f->body.size()), dim3(FASTA_TPB), 0, f->st, reinterpret_cast<const uint4 *>(f->d_text.p + 16), f->mis, f->n_bytes, (const int2 *)f->d_body.p, nchar, f->d_rows.p, f->pitch);
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev[5], f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  float ms = 0; HIPCHK(f, hipEventElapsedTime(&ms, f->ev[4], f->ev[5])); f->ms[1] += ms;
  f->n_rows = (int)f->body.size();
  *d_rows = f->d_rows.p; *n_rows = f->n_rows;
  return 0;
}

int uvaia_gpu_fasta_rows_host(uvaia_gpu_fasta *f, void *out)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (f->n_rows && !out) return fasta_fail(f, UVAIA_GPU_EINVAL, "NULL rows");
  if (!f->n_rows) return 0;
  HIPCHK(f, hipSetDevice(f->device));
  HIPCHK(f, hipMemcpy(out, f->d_rows.p, (size_t)f->n_rows * f->pitch, hipMemcpyDeviceToHost));
  return 0;
}

int uvaia_gpu_fasta_acgt(uvaia_gpu_fasta *f, int *acgt)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (f->n_rec && !acgt) return fasta_fail(f, UVAIA_GPU_EINVAL, "NULL counts");
  if (!f->n_rec) return 0;
  HIPCHK(f, hipSetDevice(f->device));
  if (int rc = f->d_acgt.reserve(f, (size_t)f->max_records)) return rc;
  HIPCHK(f, hipEventRecord(f->ev_seq[0], f->st));
  hipLaunchKernelGGL(fasta_acgt_kernel, dim3((unsigned)((f->n_rec + FASTA_TPB / 64 - 1) / (FASTA_TPB / 64))), dim3(FASTA_TPB), 0, f->st, reinterpret_cast<const uint4 *>(f->d_text.p + 16), f->mis, f->n_bytes, f->n_rec,
                     (const FastaRec *)f->d_rec.p, f->d_acgt.p);
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev_seq[1], f->st));
  HIPCHK(f, hipMemcpyAsync(acgt, f->d_acgt.p, (size_t)f->n_rec * sizeof(int), hipMemcpyDeviceToHost, f->st));
  HIPCHK(f, hipStreamSynchronize(f->st));
  float ms = 0; HIPCHK(f, hipEventElapsedTime(&ms, f->ev_seq[0], f->ev_seq[1])); f->ms_seq[0] += ms;
  return 0;
}

int uvaia_gpu_fasta_sequences(uvaia_gpu_fasta *f, const int *record, int n_sel, const void **d_bytes, int64_t *offsets)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (n_sel < 0 || !d_bytes || !offsets) return fasta_fail(f, UVAIA_GPU_EINVAL, "bad sequences arguments");
  *d_bytes = nullptr; offsets[0] = 0;
  f->seq_bytes = -1;
  // the selection: inside the last scan, no record twice (two blocks would write one range, and the offsets would not be a partition)
  if (n_sel > f->n_rec) return fasta_fail(f, UVAIA_GPU_EINVAL, "%d sequences asked for, the last scan returned %d records", n_sel, f->n_rec);
  f->chosen.assign((size_t)f->n_rec, 0);
  f->body.clear(); f->seqoff.assign(1, 0);
  for (int k = 0; k < n_sel; k++) {
    const int r = record ? record[k] : k;
    if (r < 0 || r >= f->n_rec) return fasta_fail(f, UVAIA_GPU_EINVAL, "record[%d] = %d: the last scan returned %d records", k, r, f->n_rec);
    if (f->chosen[(size_t)r]) return fasta_fail(f, UVAIA_GPU_EINVAL, "record[%d] = %d is in the selection twice", k, r);
    f->chosen[(size_t)r] = 1;
    f->body.push_back(make_int2((int)f->rec[(size_t)r].body_off, (int)f->rec[(size_t)r].body_len));
    f->seqoff.push_back(f->seqoff.back() + (long long)f->rec[(size_t)r].seq_len);
  }
  const long long total = f->seqoff.back();
  for (int k = 0; k <= n_sel; k++) offsets[k] = (int64_t)f->seqoff[(size_t)k];
  HIPCHK(f, hipSetDevice(f->device));
  if (int rc = f->d_seq.reserve(f, ((size_t)total + FASTA_SEQ_GUARD + 15) & ~(size_t)15)) return rc;
  HIPCHK(f, hipMemsetAsync(f->d_seq.p + total, 0xEE, FASTA_SEQ_GUARD, f->st));
  if (n_sel) {
    if (int rc = f->d_body.reserve(f, (size_t)n_sel)) return rc;
    if (int rc = f->d_seqoff.reserve(f, (size_t)n_sel + 1)) return rc;
    HIPCHK(f, hipMemcpyAsync(f->d_body.p, f->body.data(), (size_t)n_sel * sizeof(int2), hipMemcpyHostToDevice, f->st));
    HIPCHK(f, hipMemcpyAsync(f->d_seqoff.p, f->seqoff.data(), ((size_t)n_sel + 1) * sizeof(long long), hipMemcpyHostToDevice, f->st));
    HIPCHK(f, hipEventRecord(f->ev_seq[2], f->st));
    hipLaunchKernelGGL(fasta_sequences_kernel, dim3((unsigned)n_sel), dim3(FASTA_TPB), 0, f->st, reinterpret_cast<const uint4 *>(f->d_text.p + 16), f->mis, f->n_bytes, (const int2 *)f->d_body.p,
                       (const long long *)f->d_seqoff.p, total, f->d_seq.p);
    HIPCHK(f, hipGetLastError());
    HIPCHK(f, hipEventRecord(f->ev_seq[3], f->st));
  }
  HIPCHK(f, hipStreamSynchronize(f->st));
  if (n_sel) { float ms = 0; HIPCHK(f, hipEventElapsedTime(&ms, f->ev_seq[2], f->ev_seq[3])); f->ms_seq[1] += ms; }
  f->seq_bytes = total;
  *d_bytes = f->d_seq.p;
  return 0;
}

int uvaia_gpu_fasta_sequences_host(uvaia_gpu_fasta *f, void *out, size_t n_bytes)
{
  if (!f) return UVAIA_GPU_EINVAL;
  if (f->seq_bytes < 0) return fasta_fail(f, UVAIA_GPU_EINVAL, "no sequences were made since the last scan");
  if (!out || n_bytes != (size_t)f->seq_bytes + FASTA_SEQ_GUARD) return fasta_fail(f, UVAIA_GPU_EINVAL, "the sequences and their guard are %zu bytes (%zu given)", (size_t)f->seq_bytes + FASTA_SEQ_GUARD, n_bytes);
  HIPCHK(f, hipSetDevice(f->device));
  HIPCHK(f, hipMemcpy(out, f->d_seq.p, n_bytes, hipMemcpyDeviceToHost));
  return 0;
}

void uvaia_gpu_fasta_sequences_ms(uvaia_gpu_fasta *f, double out[2], int reset)
{
  if (!f) return;
  if (out) { out[0] = f->ms_seq[0]; out[1] = f->ms_seq[1]; }
  if (reset) f->ms_seq[0] = f->ms_seq[1] = 0.;
}

void uvaia_gpu_fasta_kernel_ms(uvaia_gpu_fasta *f, double out[2], int reset)
{
  if (!f) return;
  if (out) { out[0] = f->ms[0]; out[1] = f->ms[1]; }
  if (reset) f->ms[0] = f->ms[1] = 0.;
}

size_t uvaia_gpu_fasta_chunk_bytes(void) { return (size_t)FASTA_CHUNK; }

void *uvaia_gpu_fasta_pinned_alloc(size_t bytes)
{
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}

void uvaia_gpu_fasta_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

}  // extern "C"
