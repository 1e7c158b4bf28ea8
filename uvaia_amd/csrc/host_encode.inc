// host_encode.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): resident tiles written in the compact form of a
// packed database (kernels_encode.inc), in two steps because the sizes of the records are only known after the count pass:
// uvaia_gpu_db_encode_compact leaves the plan (offsets on the device, the tile range, the state of the database it was made for),
// uvaia_gpu_db_encoded_records runs the emit pass for it and copies the records to the host.

extern "C" {

int uvaia_gpu_db_encode_compact(uvaia_gpu_ctx *c, size_t first_tile, size_t n_tiles, const void *base, uint64_t *head_idx, uint64_t *lit_idx, int *non_n)
{
  if (!c || !base || !head_idx || !lit_idx || !non_n) return UVAIA_GPU_EINVAL;
  auto &k = c->enc;
  k.plan = false;
  if (c->acgt) return fail(c, UVAIA_GPU_ESTATE, "the interchange form is the four IUPAC planes: encode from a default-mode context");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard holds its own pieces only: encode from a plain context");
  if (c->nchar > UVAIA_GPU_COMPACT_MAX_NCHAR) return fail(c, UVAIA_GPU_ESTATE, "alignments of more than %d sites have no compact form (%d sites)", UVAIA_GPU_COMPACT_MAX_NCHAR, c->nchar);
  if ((first_tile + n_tiles) * 64 > ((c->db_n + 63) / 64) * 64) return fail(c, UVAIA_GPU_EINVAL, "tiles %zu..%zu lie outside the database", first_tile, first_tile + n_tiles);
  head_idx[0] = lit_idx[0] = 0;
  const size_t lanes = n_tiles * 64, W4 = (size_t)c->W4;
  if (n_tiles) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));                 // as uvaia_gpu_db_export; a buffer that grows below is read by nothing queued
    for (Event &e : k.ev) if (int rc = e.make(c)) return rc;
    if (int rc = k.base.reserve(c, W4 * 4)) return rc;
    if (int rc = k.cnt_h.reserve(c, lanes)) return rc;
    if (int rc = k.cnt_l.reserve(c, lanes)) return rc;
    if (int rc = k.hidx.reserve(c, lanes + 1)) return rc;
    if (int rc = k.lidx.reserve(c, lanes + 1)) return rc;
    hipStream_t s = c->st.stream;
    HIPCHK(c, hipMemcpyAsync(k.base, base, W4 * 4 * sizeof(uint4), hipMemcpyHostToDevice, s));
    const uint4 *tiles = c->db.planes.p + first_tile * W4 * 4 * 64;
    const unsigned long long n_valid = c->db_n > first_tile * 64 ? std::min<unsigned long long>(lanes, c->db_n - first_tile * 64) : 0ull;
    HIPCHK(c, hipEventRecord(k.ev[0], s));
    hipLaunchKernelGGL(encode_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, tiles, k.base, c->W4, (c->nchar + 31) / 32, n_valid, k.cnt_h, k.cnt_l);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(encode_prefix_kernel, dim3(1), dim3(1024), 0, s, k.cnt_h, k.cnt_l, (unsigned long long)lanes, k.hidx, k.lidx);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(k.ev[1], s));
    HIPCHK(c, hipMemcpyAsync(head_idx, k.hidx, (lanes + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(lit_idx, k.lidx, (lanes + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(non_n, c->db.nonn + first_tile * 64, lanes * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, k.ev[0], k.ev[1]) == hipSuccess) k.ms[0] += ms;
  }
  k.first_tile = first_tile; k.n_tiles = n_tiles; k.db_gen = c->db_gen;
  k.n_heads = head_idx[lanes]; k.n_lits = lit_idx[lanes];
  k.plan = true;
  return 0;
}

int uvaia_gpu_db_encoded_records(uvaia_gpu_ctx *c, uint32_t *heads, void *lits)
{
  if (!c) return UVAIA_GPU_EINVAL;
  auto &k = c->enc;
  if (!k.plan) return fail(c, UVAIA_GPU_ESTATE, "no compact records are planned: uvaia_gpu_db_encode_compact comes first");
  if (k.db_gen != c->db_gen) { k.plan = false; return fail(c, UVAIA_GPU_ESTATE, "the database changed since uvaia_gpu_db_encode_compact: encode its tiles again"); }
  if ((k.n_heads && !heads) || (k.n_lits && !lits)) return fail(c, UVAIA_GPU_EINVAL, "NULL record arrays");
  if (!k.n_tiles || !k.n_heads) return 0;                           // (literal words belong to literal heads: none without a head)
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->st.stream;
  HIPCHK(c, hipStreamSynchronize(s));
  if (int rc = k.heads.reserve(c, (size_t)k.n_heads)) return rc;
  if (int rc = k.lits.reserve(c, (size_t)k.n_lits + 1)) return rc;
  const size_t W4 = (size_t)c->W4, lanes = k.n_tiles * 64;
  const uint4 *tiles = c->db.planes.p + k.first_tile * W4 * 4 * 64;
  const unsigned long long n_valid = c->db_n > k.first_tile * 64 ? std::min<unsigned long long>(lanes, c->db_n - k.first_tile * 64) : 0ull;
  HIPCHK(c, hipEventRecord(k.ev[2], s));
  hipLaunchKernelGGL(encode_emit_kernel, dim3((unsigned)k.n_tiles), dim3(64), 0, s, tiles, k.base, c->W4, (c->nchar + 31) / 32, n_valid, k.hidx, k.lidx, k.heads, k.lits);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(k.ev[3], s));
  HIPCHK(c, hipMemcpyAsync(heads, k.heads, (size_t)k.n_heads * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (k.n_lits) HIPCHK(c, hipMemcpyAsync(lits, k.lits, (size_t)k.n_lits * sizeof(uint4), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, k.ev[2], k.ev[3]) == hipSuccess) k.ms[1] += ms;
  return 0;
}

void uvaia_gpu_encode_ms(uvaia_gpu_ctx *c, double out[2], int reset)
{
  if (!c) return;
  for (int i = 0; i < 2; i++) { if (out) out[i] = c->enc.ms[i]; if (reset) c->enc.ms[i] = 0.; }
}

}  // extern "C"
