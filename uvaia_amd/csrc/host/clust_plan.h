/*
 * clust_plan.h -- which residency mode `uvaiaclust --packed` asks of the clusterer (include/uvaia_cluster.h): every pushed row kept, or the
 * medoids only.  Own code, no counterpart in the reference.  Pure host arithmetic, no GPU.
 */
#ifndef UVAIA_HOST_CLUST_PLAN_H
#define UVAIA_HOST_CLUST_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The capacity schedule of the keep-everything row store (ensure_rows of uvaia_cluster.hip), replayed for n_rows sequences pushed push_rows at
 * a time: the capacity starts at 0; a push that needs more rows than there are raises it to max (rows needed, 2 x capacity, 1024); while
 * the store grows the old and the new array exist together, so that step holds (old + new capacity) x row_bytes.  (Pushes of 4 096 give
 * capacities 4 096 x 2^k.)  *peak_bytes (nullable) = the largest such step, or the final store if it is larger: what the store needs at once
 * to reach n_rows.  Saturates at UINT64_MAX. */
int uvclust_store_peak (uint64_t n_rows, uint64_t push_rows, uint64_t row_bytes, uint64_t *peak_bytes);

/* 0 = keep every row (the default mode), 1 = keep medoids: the store's peak above is more than free_bytes.  free_bytes 0 = unknown: 0, the
 * default mode, as `uvaia` treats an unknown amount of free memory as "resident".  -1 for push_rows or row_bytes below 1.  The rule counts
 * row text only: the 16 bytes or so per sequence next to it are there in either mode. */
int uvclust_choose_keep_medoids (uint64_t n_rows, uint64_t push_rows, uint64_t row_bytes, uint64_t free_bytes);

#ifdef __cplusplus
}
#endif
#endif
