/*
 * uvdb_window.h -- the window plan of `uvaia --packed --window`: a packed database (uvdb.h) that does not fit device memory is searched
 * a window of references at a time.  Own code, no counterpart in the reference: it stands where the slot-filling loop of
 * src/nearest.c:251-286 decides how many references the next batch holds.  Pure host arithmetic, no GPU.
 *
 * Positions are those of the KEPT stream: the references of the file in order, without the ones -x leaves out (keep[i] = file position
 * of the i-th kept reference, increasing; keep == NULL = every reference is kept).
 */
#ifndef UVAIA_HOST_UVDB_WINDOW_H
#define UVAIA_HOST_UVDB_WINDOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* window_request references rounded up to a multiple of lcm (pool, 64): of 64 because packed tiles only follow whole tiles, of the pool
 * because a pool boundary retakes the snapshot of the tolerances (src/nearest.c:290-291) and the pools must be the ones a search of the
 * whole stream cuts.  (A query set without constant-and-complete columns does not notice pools; the rule is the same for it, so there is
 * one behaviour.)  *n_windows = windows that cover n_kept references (0 for none).  0, or -1 for a pool or a request below 1 and for a
 * window beyond 2^31 - 64 references (the engine counts a window in an int). */
int uvdb_window_plan (uint64_t n_kept, uint64_t pool, uint64_t window_request, uint64_t *window, uint64_t *n_windows);

/* Kept-stream positions [a, b), a < b: the contiguous file tiles that hold them (*first_tile, *n_tiles) and, in sel_out[0 .. b - a)
 * (may be NULL), the position of each within those tiles -- strictly increasing, below 64 * *n_tiles.  0, or -1 for an empty range and
 * for a span beyond what an int counts. */
int uvdb_window_span (const uint64_t *keep, uint64_t a, uint64_t b, uint64_t *first_tile, uint64_t *n_tiles, int *sel_out);

/* The automatic choice.  0 = "resident, as without --window": n_kept * bytes_per_ref is at most 80 % of free_bytes.  Otherwise the
 * largest planned window (a multiple of lcm (pool, 64)) whose footprint fits those 80 %: the resident window and two staging slots, each
 * slot counted as a window's worth (a staged reference is its four planes, side row and count, never more than a resident one with its
 * derived planes).  -1 = not even the smallest window fits.  The 80 % is a safety condition -- room for the counter buffers of the
 * search and for what the runtime itself keeps -- and not a tuned figure. */
int64_t uvdb_window_choose (uint64_t n_kept, uint64_t pool, uint64_t bytes_per_ref, uint64_t free_bytes);

/* The window of `uvaia -r --device-parse`: how many accepted references are resident -- planes and text -- before they are searched and
 * cleared.  A multiple of the pool and at least one pool, because a flush must end on a pool boundary for the pools to be those of the
 * command without the option.  request rounded up to a multiple of the pool (0: the smallest multiple that is >= 65 536), lowered to the
 * largest multiple of the pool whose bytes_per_ref * window fit half of free_bytes, but never below one pool (free_bytes 0 = unknown: not
 * lowered), and to what the engine counts in an int.  0 for a pool below 1 or beyond that count. */
uint64_t uvdb_parse_window (uint64_t pool, uint64_t request, uint64_t bytes_per_ref, uint64_t free_bytes);

#ifdef __cplusplus
}
#endif
#endif
