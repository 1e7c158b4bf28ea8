/*
 * fasta_blocks_check.c -- stand-alone host program for a sanitizer run of the block reader and of fasta_scan_host, the plain C restatement of
 * the device parser's first pass (uvaia_amd/csrc/host/fasta_blocks.c), sibling of uvdb_extract_check.c.  It writes texts of its own making --
 * one line per sequence, wrapped at 60 and at 1, CRLF, no newline at the end, blank lines, spaces and tabs, lower case, bytes from 0x80 on,
 * empty names, names with '>' and header lines that begin with other bytes -- reads each through the block reader at several block sizes, from
 * the smallest that holds its longest record to one block for the whole text, and compares what comes out with the records it wrote.  Then
 * the refusals: a NUL byte, text before the first header, records without sequence, a record that does not fit a block.  No GPU is involved.
 *
 *   gcc -std=gnu11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iuvaia_amd/csrc/host -Iinclude tools/fasta_blocks_check.c \
 *       uvaia_amd/csrc/host/fasta_blocks.c uvaia_amd/csrc/host/biomcmc_lite.c -lpthread -o /tmp/fasta_blocks_check && /tmp/fasta_blocks_check /tmp/fbc
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fasta_blocks.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned
rnd (unsigned n)
{ rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned) (rng_state % n); }

struct buf { char *p; size_t n, cap; };
static void
put (struct buf *b, const void *s, size_t n)
{
  if (b->n + n + 1 > b->cap) { b->cap = 2 * (b->n + n) + 64; b->p = (char *) realloc (b->p, b->cap); if (!b->p) abort (); }
  memcpy (b->p + b->n, s, n); b->n += n;
}
static void puts_ (struct buf *b, const char *s) { put (b, s, strlen (s)); }

/* one text of n records of len sites in style, its normal form beside it; *longest = its longest record in bytes */
static void
make_text (int style, int n, int len, struct buf *text, struct buf *want, size_t *longest)
{
  static const char alpha[] = "ACGTACGTACGTACGTNRYKMSWBDHV-?XO.";
  const char *eol = (style == 3) ? "\r\n" : "\n";
  const int wrap = style == 1 ? 60 : style == 2 ? 1 : style == 3 ? 70 : len;
  *longest = 0;
  if (style == 4) puts_ (text, "\n \t\r\n");
  for (int i = 0; i < n; i++) {
    const size_t at = text->n;
    char name[64];
    if (style == 5 && i % 3 == 0) name[0] = '\0';
    else if (style == 5 && i % 3 == 1) snprintf (name, sizeof name, "a b>c %d >", i);
    else snprintf (name, sizeof name, "rec %d", i);
    if (style == 5 && i % 2) puts_ (text, "xy");
    if (style == 4 && i % 2) puts_ (text, " \t");
    puts_ (text, ">"); puts_ (text, name); puts_ (text, eol);
    puts_ (want, ">"); puts_ (want, name); puts_ (want, "\n");
    for (int s = 0; s < len; s++) {
      unsigned char c = (unsigned char) alpha[rnd (sizeof alpha - 1)];
      if (style == 6 && rnd (5) == 0) c = (unsigned char) (0x80 + rnd (128));
      unsigned char shown = c;
      if ((style == 6 || style == 4) && c >= 'A' && c <= 'Z' && rnd (2)) shown = (unsigned char) (c + 32);
      put (text, &shown, 1); put (want, &c, 1);
      if (style == 4 && rnd (7) == 0) puts_ (text, rnd (2) ? " " : "\t");
      if (style == 4 && rnd (11) == 0) puts_ (text, "\n \n\n");
      if ((s + 1) % wrap == 0 && s + 1 < len) puts_ (text, eol);
    }
    if (i + 1 < n || style != 7) puts_ (text, eol);
    puts_ (want, "\n");
    if (text->n - at > *longest) *longest = text->n - at;
  }
}

static char *
slurp (const char *path, size_t *n)
{
  FILE *f = fopen (path, "rb");
  if (!f) { *n = 0; return NULL; }
  fseek (f, 0, SEEK_END); *n = (size_t) ftell (f); rewind (f);
  char *p = (char *) malloc (*n + 1);
  if (!p || fread (p, 1, *n, f) != *n) abort ();
  fclose (f);
  return p;
}

static int
refused (const char *in, const char *out, const char *text, size_t n, size_t block, const char *word)
{
  char err[1024] = "";
  FILE *f = fopen (in, "wb");
  if (!f || fwrite (text, 1, n, f) != n) abort ();
  fclose (f);
  if (fasta_blocks_normalise_host (in, block, 64, out, err, sizeof err) == 0) { printf ("accepted: %s\n", word); return 1; }
  if (!strstr (err, word)) { printf ("refused with '%s', expected '%s'\n", err, word); return 1; }
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc < 2) { fprintf (stderr, "usage: %s <prefix of scratch files>\n", argv[0]); return 2; }
  char in[1024], out[1024], err[1024];
  snprintf (in, sizeof in, "%s.in.fa", argv[1]); snprintf (out, sizeof out, "%s.out.fa", argv[1]);
  int bad = 0, runs = 0;
  static const int shape[][2] = {{1, 29903}, {3, 1000}, {63, 64}, {64, 65}, {65, 29}, {130, 29}};
  for (int style = 0; style < 8; style++) for (size_t sh = 0; sh < sizeof shape / sizeof shape[0]; sh++) {
    struct buf text = {0, 0, 0}, want = {0, 0, 0};
    size_t longest;
    if (style == 2 && shape[sh][1] > 1000) continue;
    make_text (style, shape[sh][0], shape[sh][1], &text, &want, &longest);
    FILE *f = fopen (in, "wb");
    if (!f || fwrite (text.p, 1, text.n, f) != text.n) abort ();
    fclose (f);
    /* the lead of blank lines (style 4) and the bytes in front of a later header line belong to the block that holds the record */
    const size_t least = longest + 8, sizes[] = {least, least + 1, least + 15, least + 16, least + 17, 2 * least + 3, 4096, 65536, text.n > least ? text.n : least, text.n + 100};
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; k++) {
      if (sizes[k] < least) continue;
      for (int cap = 1; cap <= 64; cap *= 8) {
        if (fasta_blocks_normalise_host (in, sizes[k], cap, out, err, sizeof err)) { printf ("style %d, %d x %d, block %zu, cap %d: %s\n", style, shape[sh][0], shape[sh][1], sizes[k], cap, err); bad++; continue; }
        size_t n;
        char *got = slurp (out, &n);
        if (n != want.n || memcmp (got, want.p, n)) { printf ("style %d, %d x %d, block %zu, cap %d: the records differ\n", style, shape[sh][0], shape[sh][1], sizes[k], cap); bad++; }
        free (got);
        runs++;
      }
    }
    free (text.p); free (want.p);
  }
  bad += refused (in, out, ">a\nAC\0GT\n>b\nAC\n", 16, 64, "a NUL byte");
  bad += refused (in, out, "ACGT\n>a\nAC\n", 11, 64, "before the first header");
  bad += refused (in, out, ">a\nAC\n>b\n>c\nAC\n", 15, 64, "without sequence");
  bad += refused (in, out, ">a\nAC\n>b\n", 9, 64, "without sequence");
  bad += refused (in, out, ">a\nAC\n>long one\nACGTACGTACGTACGTACGT\n>c\nAC\n", 43, 24, "'long one' at byte 6 of the text does not fit");
  remove (in); remove (out);
  if (bad) { printf ("fasta_blocks_check: %d FAILED\n", bad); return 1; }
  printf ("fasta_blocks_check: ok (%d runs)\n", runs);
  return 0;
}
