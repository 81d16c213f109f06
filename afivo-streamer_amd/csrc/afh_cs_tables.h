/* AFH_COARSE_DIRECT tables of the 2-D library: the eigenbasis and the
 * eigenvalues of one dimension's folded 1-D operator (host code of
 * afh2d.hip; tests/cs_tables_probe.c reaches it on the CPU).
 *
 * A walled dimension: h tridiag(1, -2, 1) with end diagonals -h (Neumann) /
 * -3h (Dirichlet), diagonalised by a cosine / sine basis (same as the 3-D
 * AFH_COARSE_DIRECT tables).
 *
 * A periodic dimension: the circulant h tridiag(1, -2, 1) with corners h (on
 * 2 points the one neighbour twice), diagonalised by the orthonormal real
 * Fourier basis: column 0 the constant, columns 2m-1 / 2m the cos / sin of
 * 2 pi m i / n, the last column the alternating vector when n is even;
 * eigenvalues h (2 cos(2 pi m / n) - 2). The bc types are not read.
 *
 * q[i * n + p]: component i of eigenvector p; e[p] its eigenvalue. C99 and
 * C++. */
#ifndef AFH_CS_TABLES_H
#define AFH_CS_TABLES_H

#include <math.h>

#include "../../include/afivo_hip.h"

static inline void afh2_cs_tables(int n, int bc_lo, int bc_hi, int periodic, double h,
                                  double *q, double *e) {
  const double pi = 3.14159265358979323846;
  if (periodic) {
    for (int p = 0; p < n; p++) {
      const int m = (p + 1) / 2; /* 0, 1, 1, 2, 2, ... */
      const int is_sin = p > 0 && (p & 1) == 0;
      const double th = 2 * pi * m / n;
      double nrm2 = 0.0;
      for (int i = 0; i < n; i++) {
        /* (2 m = n: cos(pi i) alternates; its sin partner does not exist as
           p stops at n - 1) */
        const double v = is_sin ? sin(th * i) : cos(th * i);
        q[i * n + p] = v;
        nrm2 = nrm2 + v * v;
      }
      const double inv = 1 / sqrt(nrm2);
      for (int i = 0; i < n; i++) q[i * n + p] = q[i * n + p] * inv;
      e[p] = h * (2 * cos(th) - 2);
    }
    return;
  }
  const int dlo = bc_lo == AFH_BC_DIRICHLET, dhi = bc_hi == AFH_BC_DIRICHLET;
  for (int p = 0; p < n; p++) {
    double th;
    if (dlo == dhi) th = pi * (p + dlo) / n;
    else th = pi * (p + 0.5) / n;
    double nrm2 = 0.0;
    for (int i = 0; i < n; i++) {
      const double v = dlo ? sin(th * (i + 0.5)) : cos(th * (i + 0.5));
      q[i * n + p] = v;
      nrm2 = nrm2 + v * v;
    }
    const double inv = 1 / sqrt(nrm2);
    for (int i = 0; i < n; i++) q[i * n + p] = q[i * n + p] * inv;
    e[p] = h * (2 * cos(th) - 2);
  }
}

#endif
