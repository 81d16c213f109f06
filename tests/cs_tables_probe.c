/* Test probe: the AFH_COARSE_DIRECT tables of the 2-D library
 * (csrc/afh_cs_tables.h, afh2_cs_tables) for one dimension, written to
 * stdout (tests/test_periodic2d_cpu.py compiles and runs it).
 * Usage: cs_tables_probe n bc_lo bc_hi periodic h > tables
 * Output: float64 q[n][n] (q[i][p]: component i of eigenvector p), e[n]. */
#include <stdio.h>
#include <stdlib.h>

#include "../afivo-streamer_amd/csrc/afh_cs_tables.h"

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int n = atoi(argv[1]);
  if (n < 1) return 2;
  double *q = (double *)calloc((size_t)n * n + n, sizeof(double));
  if (!q) return 3;
  afh2_cs_tables(n, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atof(argv[5]), q,
                 q + (size_t)n * n);
  fwrite(q, sizeof(double), (size_t)n * n + n, stdout);
  free(q);
  return 0;
}
