/*
 * uvdb_window.c -- see uvdb_window.h.  Own code.
 */
#include "uvdb_window.h"

#define WINDOW_MAX ((uint64_t) 0x7FFFFFFF - 63)

static uint64_t
window_unit (uint64_t pool)
{ /* lcm (pool, 64) */
  uint64_t a = pool, b = 64;
  while (b) { const uint64_t t = a % b; a = b; b = t; }
  return pool / a * 64;
}

int
uvdb_window_plan (uint64_t n_kept, uint64_t pool, uint64_t window_request, uint64_t *window, uint64_t *n_windows)
{
  if (pool < 1 || window_request < 1 || pool > WINDOW_MAX || window_request > WINDOW_MAX) return -1;
  const uint64_t unit = window_unit (pool), w = (window_request + unit - 1) / unit * unit;
  if (w > WINDOW_MAX) return -1;
  if (window) *window = w;
  if (n_windows) *n_windows = (n_kept + w - 1) / w;
  return 0;
}

int
uvdb_window_span (const uint64_t *keep, uint64_t a, uint64_t b, uint64_t *first_tile, uint64_t *n_tiles, int *sel_out)
{
  if (b <= a) return -1;
  const uint64_t lo = keep ? keep[a] : a, hi = keep ? keep[b - 1] : b - 1;
  if (hi < lo) return -1;
  const uint64_t t0 = lo / 64, nt = hi / 64 - t0 + 1;
  if (nt > WINDOW_MAX / 64) return -1;
  if (first_tile) *first_tile = t0;
  if (n_tiles) *n_tiles = nt;
  if (sel_out) for (uint64_t k = a; k < b; k++) sel_out[k - a] = (int) ((keep ? keep[k] : k) - t0 * 64);
  return 0;
}

int64_t
uvdb_window_choose (uint64_t n_kept, uint64_t pool, uint64_t bytes_per_ref, uint64_t free_bytes)
{
  if (pool < 1 || pool > WINDOW_MAX || bytes_per_ref < 1) return -1;
  const uint64_t budget = free_bytes / 5 * 4;
  if (n_kept <= budget / bytes_per_ref) return 0;
  const uint64_t unit = window_unit (pool);
  uint64_t w = budget / bytes_per_ref / 3 / unit * unit;       /* the window and two staging slots */
  if (w > WINDOW_MAX) w = WINDOW_MAX / unit * unit;
  return w ? (int64_t) w : -1;
}

uint64_t
uvdb_parse_window (uint64_t pool, uint64_t request, uint64_t bytes_per_ref, uint64_t free_bytes)
{
  if (pool < 1 || pool > WINDOW_MAX) return 0;
  if (!request) request = 65536;
  if (request > WINDOW_MAX) request = WINDOW_MAX;
  uint64_t w = (request + pool - 1) / pool * pool;
  if (w > WINDOW_MAX) w = WINDOW_MAX / pool * pool;
  if (free_bytes && bytes_per_ref) {
    const uint64_t fit = free_bytes / 2 / bytes_per_ref / pool * pool;
    if (fit < w) w = fit;
  }
  return w < pool ? pool : w;
}
