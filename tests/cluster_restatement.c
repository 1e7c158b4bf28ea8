/*
 * cluster_restatement.c -- CPU restatement of what the reference's `uvaiaclust` computes (src/cluster.c, src/fastaseq.c:23-258,
 * 489-560, 642-648, src/utils.c:255-295), loop for loop, for the tests and the CPU baseline of tools/cluster_bench.py.  Not part
 * of the product.  Built by the tests with `cc -O2 -fopenmp -shared -fPIC`.
 *
 * Where it departs from a literal copy, it does so by the defined choices of include/uvaia_cluster.h:
 *   - the site tables are those the program leaves uninitialised (src/utils.c:255-256: only index 0 set), so a pair is valid when
 *     neither byte is NUL; bytes 0 and >= 0x80 are refused by the caller;
 *   - the window of src/fastaseq.c:158 that runs past the end of the rows stops at their end: sites >= nchar never count;
 *   - the out-of-bounds write of src/fastaseq.c:160 is not made;
 *   - qsort is a stable merge sort (ties keep their order);
 *   - an empty absorbed queue merges as a no-op, an empty absorbing queue takes the other list as it is sorted;
 *   - names are push ordinals.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef struct {
  int name;          /* push ordinal */
  const char *seq;   /* nchars bytes */
  int *score, n_score;
  int *nn, n_nn, nn_cap;
} fastaseq;

typedef struct {
  fastaseq **fs;
  int n_fs, n_score, mindist, trim, nchars, n_idx;
  const char *reference;
  int *idx;
} cluster;

/* src/utils.c:255-283 without initialise_acgt(): is_indel[] is zero except index 0 */
static int is_site_pair_valid (char s1, char s2) { return s1 != 0 && s2 != 0; }

/* src/fastaseq.c:23-40 */
static int
compare_fastaseq_score (const fastaseq *a, const fastaseq *b)
{
  for (int i = 0; i < b->n_score + 2; i++) { int res = b->score[i] - a->score[i]; if (res) return res; }
  return -1;
}

static int
compare_fastaseq (const fastaseq *a, const fastaseq *b)
{
  int res_i = b->n_nn - a->n_nn;
  if (res_i) return res_i;
  return compare_fastaseq_score (a, b);
}

/* stable merge sort: b goes before a only when cmp(b, a) < 0 and cmp(a, b) > 0 (the comparators return -1 on ties) */
static void
stable_sort (fastaseq **v, int n, int (*cmp) (const fastaseq *, const fastaseq *))
{
  if (n < 2) return;
  fastaseq **tmp = (fastaseq **) malloc ((size_t) n * sizeof (fastaseq *)), **src = v, **dst = tmp;
  for (int width = 1; width < n; width *= 2) {
    for (int lo = 0; lo < n; lo += 2 * width) {
      int mid = lo + width < n ? lo + width : n, hi = lo + 2 * width < n ? lo + 2 * width : n, a = lo, b = mid, o = lo;
      while (a < mid && b < hi) dst[o++] = cmp (src[a], src[b]) > 0 ? src[b++] : src[a++];
      while (a < mid) dst[o++] = src[a++];
      while (b < hi) dst[o++] = src[b++];
    }
    fastaseq **t = src; src = dst; dst = t;
  }
  if (src != v) memcpy (v, src, (size_t) n * sizeof (fastaseq *));
  free (tmp);
}

static void
nn_append (fastaseq *f, int name)
{
  if (f->n_nn == f->nn_cap) { f->nn_cap = f->nn_cap ? 2 * f->nn_cap : 4; f->nn = (int *) realloc (f->nn, (size_t) f->nn_cap * sizeof (int)); }
  f->nn[f->n_nn++] = name;
}

/* src/fastaseq.c:522-537 */
static void
quick_pairwise_score_reference (const char *s1, const char *s2, int nsites, int *score, int n_score, int *counter)
{
  int i;
  score[0] = 0;
  for (i = 1; i <= n_score; i++) score[i] = -1;
  for (i = 0; i < nsites; i++) {
    if (!is_site_pair_valid (s1[i], s2[i])) continue;
    score[0]++;
    if (s1[i] == s2[i]) score[0]--;
    else counter[i]++;
    if ((n_score) && (score[0]) && (score[0] <= n_score) && (score[score[0]] < 0)) score[score[0]] = i;
  }
}

/* src/fastaseq.c:539-551 */
static void
quick_pairwise_score_truncated (const char *s1, const char *s2, int nsites, int maxdist, int *score)
{
  int i;
  score[0] = 0;
  for (i = 0; (i < nsites) && (score[0] < maxdist); i++) {
    if (!is_site_pair_valid (s1[i], s2[i])) continue;
    score[0]++;
    if (s1[i] == s2[i]) score[0]--;
  }
}

/* src/fastaseq.c:553-560 */
static void
quick_pairwise_score_truncated_idx (const char *s1, const char *s2, int nsites, int maxdist, int *score, const int *idx)
{
  *score = 0;
  for (int i = 0; (i < nsites) && (score[0] < maxdist); i++) if (s1[idx[i]] != s2[idx[i]]) (*score)++;
}

/* src/fastaseq.c:642-648 */
static int
quick_count_sequence_non_N (const char *s, int nsites)
{
  int non_n = 0;
  for (int i = 0; i < nsites; i++) non_n += s[i] != 0;
  return non_n;
}

/* src/fastaseq.c:75-93 (the sequence is shared, never freed here) */
static void
update_fasta_seq (fastaseq *to, const char *seq, int name, const int *score)
{
  to->seq = seq;
  if (to->name >= 0) nn_append (to, to->name);
  to->name = name;
  for (int i = 0; i < to->n_score + 2; i++) to->score[i] = score[i];
}

/* src/fastaseq.c:172-193 */
static void
add_seq_to_cluster (cluster *clust, int idx, const char *seq, int name, const int *score)
{
  if (idx >= clust->n_fs) {
    idx = clust->n_fs;
    clust->fs = (fastaseq **) realloc (clust->fs, (size_t) (++clust->n_fs) * sizeof (fastaseq *));
    fastaseq *f = (fastaseq *) calloc (1, sizeof (fastaseq));
    f->name = -1; f->n_score = clust->n_score;
    f->score = (int *) calloc ((size_t) clust->n_score + 2, sizeof (int));
    clust->fs[idx] = f;
    update_fasta_seq (f, seq, name, score);
    return;
  }
  if (score[clust->n_score + 1] > clust->fs[idx]->score[clust->n_score + 1]) { update_fasta_seq (clust->fs[idx], seq, name, score); return; }
  nn_append (clust->fs[idx], name);
}

/* src/fastaseq.c:140-170 */
static void
check_seq_against_cluster (cluster *clust, const char *seq, int name)
{
  int i, minloc = 0;
  const size_t scorelength = (size_t) clust->n_score + 2;
  int *score = (int *) malloc (scorelength * sizeof (int));
  score[scorelength - 1] = quick_count_sequence_non_N (seq, clust->nchars);
  quick_pairwise_score_reference (seq + clust->trim, clust->reference + clust->trim, clust->nchars - 2 * clust->trim, score, clust->n_score, clust->idx);
  for (i = 0; i < clust->n_fs; i++) if (abs (score[0] - clust->fs[i]->score[0]) <= clust->mindist) {
    if (clust->n_score) minloc = (score[1] < clust->fs[i]->score[1] ? score[1] : clust->fs[i]->score[1]) - 1;
    else minloc = 0;
    if (minloc < 0) minloc = 0;
    /* the window [trim + minloc, nchars - trim + minloc) runs past the buffer for minloc > trim: those sites never count */
    int nsites = clust->nchars - 2 * clust->trim;
    if (minloc > clust->trim) nsites -= minloc - clust->trim;
    quick_pairwise_score_truncated (seq + clust->trim + minloc, clust->fs[i]->seq + clust->trim + minloc, nsites, clust->mindist + 1, score);
    if (score[0] <= clust->mindist) {   /* (src/fastaseq.c:160 writes score[scorelength]: out of bounds, no effect) */
      add_seq_to_cluster (clust, i, seq, name, score);
      free (score);
      return;
    }
  }
  add_seq_to_cluster (clust, i, seq, name, score);
  free (score);
}

/* src/fastaseq.c:127-138 */
static void
generate_idx_from_cluster_list (cluster **clust, int n_clust, int min_freq)
{
  int c, i, n_i = 0;
  for (c = 1; c < n_clust; c++) for (i = 0; i < clust[0]->n_idx; i++) clust[0]->idx[i] += clust[c]->idx[i];
  for (i = 0; i < clust[0]->n_idx; i++) if (clust[0]->idx[i] > min_freq) clust[0]->idx[n_i++] = i;
  for (c = 0; c < n_clust; c++) clust[c]->n_idx = n_i;
  for (c = 1; c < n_clust; c++) for (i = 0; i < n_i; i++) clust[c]->idx[i] = clust[0]->idx[i];
}

/* src/fastaseq.c:195-260 */
static int
merge_clusters (cluster *clust1, cluster *clust2)
{
  int i, j, count = 0, first = 0, last = 0, c2s, c1_n_fs = clust1->n_fs, *dst, maxdst, *idx2, score[1];
  if (!clust2->n_fs) return 0;                                   /* defined choice: the reference dereferences clust2->fs[0] */
  stable_sort (clust1->fs, clust1->n_fs, compare_fastaseq_score);
  stable_sort (clust2->fs, clust2->n_fs, compare_fastaseq_score);
  if (!c1_n_fs) {                                                /* defined choice: every element of clust2 is appended */
    clust1->fs = clust2->fs; clust1->n_fs = clust2->n_fs; clust2->fs = NULL; clust2->n_fs = 0;
    return 0;
  }
  maxdst = clust1->fs[0]->score[0];
  dst = (int *) malloc ((size_t) (maxdst + 1) * sizeof (int));
  for (i = 0; i <= maxdst; i++) dst[i] = -1;
  for (i = 0; i < c1_n_fs; i++) if (dst[clust1->fs[i]->score[0]] < 0) dst[clust1->fs[i]->score[0]] = i;
  idx2 = (int *) malloc (2 * (size_t) (clust2->fs[0]->score[0] + 1) * sizeof (int));
  for (i = 0; i < 2 * (clust2->fs[0]->score[0] + 1); i++) idx2[i] = -1;
  for (j = 0; j < clust2->n_fs; j++) if (idx2[2 * clust2->fs[j]->score[0]] < 0) {
    c2s = clust2->fs[j]->score[0];
    for (i = c2s + clust1->mindist; (i >= 0) && (i <= maxdst) && (dst[i] < 0); i++);
    if ((i >= 0) && (i <= maxdst)) first = dst[i];
    else first = 0;
    for (i = c2s - clust1->mindist - 1; (i >= 0) && (i <= maxdst) && (dst[i] < 0); i--);
    if ((i >= 0) && (i <= maxdst)) last = dst[i];
    else last = c1_n_fs;
    idx2[2 * c2s] = first;
    idx2[(2 * c2s) + 1] = last;
  }
  for (j = 0; j < clust2->n_fs; j++) {
    c2s = clust2->fs[j]->score[0];
    first = idx2[2 * c2s]; last = idx2[(2 * c2s) + 1];
    for (i = first; i < last; i++) if (abs (c2s - clust1->fs[i]->score[0]) <= clust1->mindist) {
      fastaseq *f1 = clust1->fs[i], *f2 = clust2->fs[j];
      quick_pairwise_score_truncated_idx (f1->seq + clust1->trim, f2->seq + clust1->trim, clust1->n_idx, clust1->mindist + 1, score, clust1->idx);
      if (score[0] <= clust1->mindist) {
        add_seq_to_cluster (clust1, i, f2->seq, f2->name, f2->score);
        for (int k = 0; k < f2->n_nn; k++) nn_append (f1, f2->nn[k]);
        free (f2->nn); free (f2->score); free (f2);
        clust2->fs[j] = NULL;
        count++;
        break;
      }
    }
    if (i == last) {
      clust1->fs = (fastaseq **) realloc (clust1->fs, (size_t) (clust1->n_fs + 1) * sizeof (fastaseq *));
      clust1->fs[clust1->n_fs++] = clust2->fs[j];
      clust2->fs[j] = NULL;
    }
  }
  free (clust2->fs); clust2->fs = NULL; clust2->n_fs = 0;
  free (dst); free (idx2);
  return count;
}

/* The whole program after the reading (src/cluster.c:157-237) for n rows of nchar bytes (rows[i * nchar ..]) whose queues are
 * given (src/cluster.c:164-181 decide them: k mod Q within each file).  Parameters already clamped (src/cluster.c:131-132,287-289).
 * Outputs as uvaia_clust_result (include/uvaia_cluster.h).  Returns the number of clusters. */
int
rs_cluster (const char *reference, int nchar, int dist, int trim, int n_score, int n_queues, int n, const char *rows, const int *queue,
            int64_t *medoid, int64_t *offsets, int64_t *members, int *scores)
{
  const size_t pitch = (size_t) nchar + 1;
  char *store = (char *) calloc ((size_t) n * pitch + 1, 1);
  for (int i = 0; i < n; i++) for (int k = 0; k < nchar; k++) {   /* upper_kseq (src/fastaseq.c:151) */
    char ch = rows[(size_t) i * nchar + k];
    store[(size_t) i * pitch + k] = (ch >= 'a' && ch <= 'z') ? ch - 32 : ch;
  }
  char *ref = (char *) calloc (pitch, 1);
  memcpy (ref, reference, (size_t) nchar);
  cluster **cq = (cluster **) malloc ((size_t) n_queues * sizeof (cluster *));
  for (int c = 0; c < n_queues; c++) {    /* new_cluster, src/fastaseq.c:95-113 */
    cluster *k = (cluster *) calloc (1, sizeof (cluster));
    k->n_score = n_score; k->mindist = dist; k->trim = trim; k->nchars = nchar; k->reference = ref;
    k->n_idx = nchar; k->idx = (int *) calloc ((size_t) nchar, sizeof (int));
    cq[c] = k;
  }
  /* per-queue lists in push order */
  int *qoff = (int *) calloc ((size_t) n_queues + 1, sizeof (int)), *qlist = (int *) malloc ((size_t) (n ? n : 1) * sizeof (int)), *fill;
  for (int i = 0; i < n; i++) qoff[queue[i] + 1]++;
  for (int c = 0; c < n_queues; c++) qoff[c + 1] += qoff[c];
  fill = (int *) malloc ((size_t) n_queues * sizeof (int));
  memcpy (fill, qoff, (size_t) n_queues * sizeof (int));
  for (int i = 0; i < n; i++) qlist[fill[queue[i]]++] = i;
  /* src/cluster.c:183-190: the queues are independent, each takes its sequences in order */
#pragma omp parallel for schedule(dynamic, 1)
  for (int c = 0; c < n_queues; c++)
    for (int k = qoff[c]; k < qoff[c + 1]; k++) check_seq_against_cluster (cq[c], store + (size_t) qlist[k] * pitch, qlist[k]);
  generate_idx_from_cluster_list (cq, n_queues, 0);              /* src/cluster.c:208 */
  for (int c = n_queues; c > 1; c = (c / 2 + c % 2)) {           /* src/cluster.c:219-230 */
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = 0; j < c / 2; j++) merge_clusters (cq[j], cq[j + c / 2 + c % 2]);
  }
  stable_sort (cq[0]->fs, cq[0]->n_fs, compare_fastaseq);        /* src/cluster.c:233 */
  const int n_clust = cq[0]->n_fs;
  int64_t at = 0;
  for (int k = 0; k < n_clust; k++) {
    fastaseq *f = cq[0]->fs[k];
    if (medoid) medoid[k] = f->name;
    if (offsets) offsets[k] = at;
    for (int m = 0; m < f->n_nn; m++, at++) if (members) members[at] = f->nn[m];
    if (scores) for (int s = 0; s < n_score + 2; s++) scores[(size_t) k * (n_score + 2) + s] = f->score[s];
    free (f->nn); free (f->score); free (f);
  }
  if (offsets) offsets[n_clust] = at;
  for (int c = 0; c < n_queues; c++) { free (cq[c]->fs); free (cq[c]->idx); free (cq[c]); }
  free (cq); free (qoff); free (qlist); free (fill); free (store); free (ref);
  return n_clust;
}

/* read_reference_sequence (src/cluster.c:260-277) over rows already read: accumulate_reference_sequence (src/fastaseq.c:488-512)
 * while Ns remain, then replace_Ns_from_reference (src/fastaseq.c:514-520).  out: nchar bytes. */
void
rs_reference (const char *rows, int n, int nchar, char *out)
{
  int count = 0xff;
  for (int k = 0; k < n && count; k++) {
    const char *s = rows + (size_t) k * nchar;
    count = 0;
    if (!k) {
      for (int i = 0; i < nchar; i++) {
        char ch = s[i]; if (ch >= 'a' && ch <= 'z') ch -= 32;
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') { ch = 'N'; count++; }
        out[i] = ch;
      }
      continue;
    }
    for (int i = 0; i < nchar; i++) {
      char ch = s[i]; if (ch >= 'a' && ch <= 'z') ch -= 32;
      if (out[i] == 'N') {
        if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') out[i] = ch;
        else count++;
      }
    }
  }
  for (int i = 0; i < nchar; i++) if (out[i] == 'N') out[i] = 'A';
}

int
rs_threads (void)
{
#ifdef _OPENMP
  return omp_get_max_threads ();
#else
  return 1;
#endif
}
