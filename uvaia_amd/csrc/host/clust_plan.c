/*
 * clust_plan.c -- see clust_plan.h.  Own code.
 */
#include "clust_plan.h"

static uint64_t
mul_sat (uint64_t a, uint64_t b)
{
  return (b && a > UINT64_MAX / b) ? UINT64_MAX : a * b;
}

int
uvclust_store_peak (uint64_t n_rows, uint64_t push_rows, uint64_t row_bytes, uint64_t *peak_bytes)
{
  if (push_rows < 1 || row_bytes < 1) return -1;
  uint64_t cap = 0, peak_rows = 0, pushed = 0;
  while (pushed < n_rows) {
    const uint64_t n = n_rows - pushed < push_rows ? n_rows - pushed : push_rows, need = pushed + n;
    if (need > cap) {
      uint64_t to = cap > UINT64_MAX / 2 ? UINT64_MAX : 2 * cap;
      if (to < 1024) to = 1024;
      if (to < need) to = need;
      if (cap > UINT64_MAX - to) { peak_rows = UINT64_MAX; break; }
      if (cap + to > peak_rows) peak_rows = cap + to;
      cap = to;
      /* nothing grows before the capacity is used up: skip the pushes that fit */
      if (cap > need) { const uint64_t k = (cap - need) / push_rows; pushed = need + k * push_rows; continue; }
    }
    pushed = need;
  }
  if (peak_bytes) *peak_bytes = mul_sat (peak_rows, row_bytes);
  return 0;
}

int
uvclust_choose_keep_medoids (uint64_t n_rows, uint64_t push_rows, uint64_t row_bytes, uint64_t free_bytes)
{
  uint64_t peak = 0;
  if (uvclust_store_peak (n_rows, push_rows, row_bytes, &peak)) return -1;
  if (!free_bytes) return 0;
  return peak > free_bytes;
}
