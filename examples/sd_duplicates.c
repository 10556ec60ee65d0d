/*
 * sd_duplicates.c — what a library's duplicates cost, through the C ABI alone (no Python, no
 * torch): the two values core/src/library/statistics.rs:42,46 writes as 0
 * (total_object_count, total_unique_bytes) and the duplicate sets that waste the most space.
 *
 *   sd_duplicates <dir> [top_k] [--exact]
 *
 * 1. walks <dir> (regular files, sorted by path = the file_path id order of a fresh library);
 * 2. FileMetadata::new over all of them (sd_cas_file_metadata_from_paths: the cas key, the
 *    status and the fs::metadata().len() each row was decided from);
 * 3. one sd_cas_duplicate_report: grouping, copies per Object, the totals and the top_k
 *    (default 10) sets by waste = (copies - 1) * size.  Only hashed rows take part; an empty
 *    file has no cas_id and is one more Object of 0 bytes in the reference (mod.rs:246-253),
 *    which is added to total_object_count here.
 * With a trailing --exact, step 2 is sd_cas_identify_validate_paths (cas key and whole-content
 * checksum from one read of each file) and step 3 is sd_cas_duplicate_report_exact: the same
 * report, plus "exact" — the totals and top list over the sets whose checksums agree as well,
 * i.e. the files that really are byte-identical (a cas_id samples files beyond 100 KiB) — and
 * "unconfirmed", the hashed files whose checksum could not be taken.
 * Prints one JSON object.  Exit status 0 on success.
 */
#define _XOPEN_SOURCE 700
#include <errno.h>
#include <ftw.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "sd_hip_cas.h"

static char** g_paths;
static size_t g_n, g_cap;

static int visit(const char* p, const struct stat* st, int type, struct FTW* f) {
  (void)f;
  if (type != FTW_F || !S_ISREG(st->st_mode)) return 0;
  if (g_n == g_cap) {
    g_cap = g_cap ? 2 * g_cap : 1024;
    g_paths = realloc(g_paths, g_cap * sizeof *g_paths);
    if (!g_paths) return -1;
  }
  g_paths[g_n++] = strdup(p);
  return 0;
}

static int by_path(const void* a, const void* b) {
  return strcmp(*(char* const*)a, *(char* const*)b);
}

static const char* g_names[SD_CAS_STAT_COUNT] = {
    "rows", "objects", "total_bytes", "unique_bytes", "duplicate_sets", "max_copies",
    "size_mismatch_rows", "bad_rows"};

static void json_str(const char* s) {
  putchar('"');
  for (; *s; s++) {
    if (*s == '"' || *s == '\\') printf("\\%c", *s);
    else if ((unsigned char)*s < 0x20) printf("\\u%04x", (unsigned char)*s);
    else putchar(*s);
  }
  putchar('"');
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dir> [top_k] [--exact]\n", argv[0]);
    return 2;
  }
  const int exact = argc > 2 && !strcmp(argv[argc - 1], "--exact");
  if (exact) argc--;
  const size_t k = argc > 2 ? (size_t)strtoul(argv[2], NULL, 10) : 10;
  if (nftw(argv[1], visit, 64, FTW_PHYS) != 0) {
    fprintf(stderr, "walk %s: %s\n", argv[1], strerror(errno));
    return 1;
  }
  const size_t n = g_n;
  qsort(g_paths, n, sizeof *g_paths, by_path);
  sd_cas_ctx* ctx = NULL;
  int rc = sd_cas_ctx_create(0, &ctx);
  if (rc != SD_CAS_OK) {
    fprintf(stderr, "sd_cas_ctx_create: %d (%s)\n", rc, sd_cas_last_error(NULL));
    return 1;
  }
  const size_t a = n ? n : 1, ka = k ? k : 1;
  uint64_t* keys = calloc(a, 8);
  uint64_t* sizes = calloc(a, 8);
  int32_t* status = calloc(a, 4);
  uint8_t* state = calloc(a, 1);
  uint32_t* rep = calloc(a, 4);
  uint32_t* copies = calloc(a, 4);
  uint32_t* heads = calloc(ka, 4);
  uint64_t* waste = calloc(ka, 8);
  char* hex = exact ? calloc(a, 65) : NULL;
  int32_t* ck_status = exact ? calloc(a, 4) : NULL;
  uint32_t* rep_exact = exact ? calloc(a, 4) : NULL;
  if (exact) {
    if (n && (rc = sd_cas_identify_validate_paths(ctx, (const char* const*)g_paths, n, keys, status, sizes,
                                                  hex, ck_status)) != SD_CAS_OK) {
      fprintf(stderr, "identify_validate_paths: %d (%s)\n", rc, sd_cas_last_error(ctx));
      return 1;
    }
  } else if (n && (rc = sd_cas_file_metadata_from_paths(ctx, (const char* const*)g_paths, n, keys, status,
                                                        sizes)) != SD_CAS_OK) {
    fprintf(stderr, "file_metadata_from_paths: %d (%s)\n", rc, sd_cas_last_error(ctx));
    return 1;
  }
  size_t no_cas = 0, errors = 0;
  for (size_t i = 0; i < n; i++) {
    state[i] = status[i] == SD_CAS_STATUS_NO_CAS ? SD_CAS_ROW_NO_CAS
               : status[i] ? SD_CAS_ROW_ERROR : SD_CAS_ROW_HASHED;
    no_cas += state[i] == SD_CAS_ROW_NO_CAS;
    errors += state[i] == SD_CAS_ROW_ERROR;
  }
  uint64_t totals[SD_CAS_STAT_COUNT], found = 0;
  uint64_t totals_exact[SD_CAS_STAT_COUNT], found_exact = 0, unconfirmed = 0;
  uint32_t* heads_exact = exact ? calloc(ka, 4) : NULL;
  uint64_t* waste_exact = exact ? calloc(ka, 8) : NULL;
  uint32_t* copies_exact = exact ? calloc(a, 4) : NULL;
  if (exact && (rc = sd_cas_duplicate_report_exact(ctx, keys, sizes, hex, state, n, NULL, rep_exact,
                                                   copies_exact, NULL, totals_exact, &unconfirmed, k,
                                                   heads_exact, waste_exact, &found_exact)) != SD_CAS_OK) {
    fprintf(stderr, "duplicate_report_exact: %d (%s)\n", rc, sd_cas_last_error(ctx));
    return 1;
  }
  if ((rc = sd_cas_duplicate_report(ctx, keys, sizes, state, n, rep, copies, totals, k, heads, waste,
                                    &found)) != SD_CAS_OK) {
    fprintf(stderr, "duplicate_report: %d (%s)\n", rc, sd_cas_last_error(ctx));
    return 1;
  }
  const char** names = g_names;
  printf("{\"files\": %zu, \"no_cas\": %zu, \"errors\": %zu", n, no_cas, errors);
  printf(", \"total_object_count\": %llu, \"total_unique_bytes\": \"%llu\"",
         (unsigned long long)(totals[SD_CAS_STAT_OBJECTS] + no_cas),
         (unsigned long long)totals[SD_CAS_STAT_UNIQUE_BYTES]);
  printf(", \"totals\": {");
  for (int j = 0; j < SD_CAS_STAT_COUNT; j++)
    printf("%s\"%s\": %llu", j ? ", " : "", names[j], (unsigned long long)totals[j]);
  printf("}, \"top\": [");
  for (uint64_t j = 0; j < found; j++) {
    const uint32_t h = heads[j];
    char hex[17];
    sd_cas_key_to_hex(keys[h], hex);
    printf("%s{\"cas_id\": \"%s\", \"copies\": %u, \"size\": %llu, \"waste\": %llu, \"paths\": [",
           j ? ", " : "", hex, copies[h], (unsigned long long)sizes[h], (unsigned long long)waste[j]);
    int first = 1;
    for (size_t i = h; i < n; i++) {  /* the set's member paths: they follow their head */
      if (rep[i] != h) continue;
      if (!first) printf(", ");
      json_str(g_paths[i]);
      first = 0;
    }
    printf("]}");
  }
  printf("]");
  if (exact) {
    printf(", \"unconfirmed\": %llu, \"exact\": {\"totals\": {", (unsigned long long)unconfirmed);
    for (int j = 0; j < SD_CAS_STAT_COUNT; j++)
      printf("%s\"%s\": %llu", j ? ", " : "", names[j], (unsigned long long)totals_exact[j]);
    printf("}, \"top\": [");
    for (uint64_t j = 0; j < found_exact; j++) {
      const uint32_t h = heads_exact[j];
      char id[17];
      sd_cas_key_to_hex(keys[h], id);
      printf("%s{\"cas_id\": \"%s\", \"checksum\": \"%s\", \"copies\": %u, \"size\": %llu, \"waste\": %llu, "
             "\"paths\": [", j ? ", " : "", id, hex + 65 * (size_t)h, copies_exact[h],
             (unsigned long long)sizes[h], (unsigned long long)waste_exact[j]);
      int first = 1;
      for (size_t i = h; i < n; i++) {
        if (rep_exact[i] != h) continue;
        if (!first) printf(", ");
        json_str(g_paths[i]);
        first = 0;
      }
      printf("]}");
    }
    printf("]}");
  }
  printf("}\n");
  sd_cas_ctx_destroy(ctx);
  return 0;
}
