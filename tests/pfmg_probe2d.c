/* Test probe: the host set-up of csrc/afh_pfmg.h as the 2-D library calls it
 * (afh_pfmg_setup_per with ndim = 2, nz = 1) on a folded 5-point operator
 * read from stdin (7 per point, the z entries 0), the whole hierarchy
 * written to stdout (tests/test_periodic2d_cpu.py compiles and runs it).
 * Usage: pfmg_probe2d nx ny px py < a7 > hierarchy
 * Output: int32 nl, n[nl][3], cdir[nl], active[nl]; float64 w[nl],
 * A[points][27], P[points][2]. */
#include <stdio.h>

#include "../afivo-streamer_amd/csrc/afh_pfmg.h"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const int nx = atoi(argv[1]), ny = atoi(argv[2]);
  const int per[3] = {atoi(argv[3]), atoi(argv[4]), 0};
  const size_t n0 = (size_t)nx * ny;
  double *a7 = (double *)calloc(7 * n0, sizeof(double));
  if (!a7 || fread(a7, sizeof(double), 7 * n0, stdin) != 7 * n0) return 3;
  afh_pfmg h;
  if (afh_pfmg_setup_per(&h, nx, ny, 1, 2, a7, per)) return 4;
  const size_t np = h.off[h.nl];
  fwrite(&h.nl, sizeof(int), 1, stdout);
  fwrite(h.n, sizeof(int), 3 * (size_t)h.nl, stdout);
  fwrite(h.cdir, sizeof(int), (size_t)h.nl, stdout);
  fwrite(h.active, sizeof(int), (size_t)h.nl, stdout);
  fwrite(h.w, sizeof(double), (size_t)h.nl, stdout);
  fwrite(h.A, sizeof(double), 27 * np, stdout);
  fwrite(h.P, sizeof(double), 2 * np, stdout);
  afh_pfmg_free(&h);
  free(a7);
  return 0;
}
