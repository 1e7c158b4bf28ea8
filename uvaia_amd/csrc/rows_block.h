// rows_block.h -- a block of text rows handed in by device pointer (include/uvaia_gpu.h, "rows that are already in device memory"), as the
// engine (uvaia_gpu.hip: kernels_rows.inc, host_rows.inc, host_text.inc) and the clustering (uvaia_cluster.hip: uvaia_clust_push_device) take
// it: the host's check of the pointer and the device's load of 16 sites.  A block is n rows of nchar bytes, `pitch` bytes apart; nothing is
// assumed about the pitch or about the alignment of the first row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

// The block must be device memory of `device` (asked of the runtime, the pointer is not dereferenced before) and rows 0 .. last_row must lie
// inside its allocation (last_row < 0: only the pointer is looked at).  true, or false with the reason in msg.
static inline bool rows_block_ok(const void *d_rows, size_t pitch, int nchar, int device, long long last_row, char *msg, size_t msglen)
{
  if (!d_rows) { snprintf(msg, msglen, "NULL rows"); return false; }
  if (pitch < (size_t)nchar) { snprintf(msg, msglen, "pitch %zu is below the %d sites of a row", pitch, nchar); return false; }
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, d_rows) != hipSuccess) { (void)hipGetLastError(); snprintf(msg, msglen, "the rows are not in device memory"); return false; }
  if (at.type != hipMemoryTypeDevice || at.device != device) {
    snprintf(msg, msglen, "the rows must be in the memory of device %d (memory type %d, device %d)", device, (int)at.type, at.device);
    return false;
  }
  hipDeviceptr_t base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(d_rows)) != hipSuccess) { (void)hipGetLastError(); snprintf(msg, msglen, "the rows are not inside a device allocation"); return false; }
  const size_t off = (size_t)(reinterpret_cast<const char *>(d_rows) - reinterpret_cast<const char *>(base));
  if (last_row >= 0 && (off > size || (size_t)last_row > (size - off) / pitch || (size_t)last_row * pitch + (size_t)nchar > size - off)) {
    snprintf(msg, msglen, "row %lld ends beyond the device allocation the rows lie in (%zu bytes from its start, %zu in all)", last_row, off, size);
    return false;
  }
  return true;
}

// sites site0 .. site0 + 15 of a row (site0 < nchar, a multiple of 16); bytes at and beyond nchar read as the bytes of FILL.  A row that
// starts on a 16-byte boundary is read with one dwordx4 load, any other through five aligned dwords and v_alignbyte; no dword is touched that
// holds no byte of the row.
template <uint32_t FILL>
static __device__ __forceinline__ uint4 rows_load16_fill(const uint8_t *row, int nchar, int site0)
{
  const uint8_t *p = row + site0;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && site0 + 16 <= nchar) return *reinterpret_cast<const uint4 *>(p);
  const uintptr_t a = reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3, end = reinterpret_cast<uintptr_t>(row) + (size_t)nchar;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  uint32_t w[5], o[4];
#pragma unroll
  for (int i = 0; i < 5; i++) w[i] = (a + 4 * i < end) ? *reinterpret_cast<const uint32_t *>(a + 4 * i) : FILL;     // (a dword that starts inside the row)
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
  const int rem = nchar - site0;
  if (rem < 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int keep = min(max(rem - 4 * i, 0), 4);                      // bytes of this dword that belong to the row
      const uint32_t m = keep == 4 ? 0xFFFFFFFFu : ((1u << (8 * keep)) - 1u);
      o[i] = (o[i] & m) | (FILL & ~m);
    }
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}
