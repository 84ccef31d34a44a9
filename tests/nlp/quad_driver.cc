// Host driver of sparsergps_amd/csrc/sgp_quad.h (tests/test_nlp_quad.py): reads rows
// "family y pred_mean pred_var par" from standard input, one per line, and prints each row's nlp
// with %.17g -- the arithmetic k_nlp_rows runs, as a program of its own.
#include <stdio.h>

#include "../../sparsergps_amd/csrc/sgp_quad.h"

int main() {
  int fam;
  double y, mu, s2, par;
  long n = 0;
  while (scanf("%d %lf %lf %lf %lf", &fam, &y, &mu, &s2, &par) == 5) {
    if (fam != SGP_QUAD_POISSON && fam != SGP_QUAD_BERNOULLI && fam != SGP_QUAD_GAUSSIAN) {
      fprintf(stderr, "FAIL: unknown family %d on row %ld\n", fam, n);
      return 1;
    }
    printf("%.17g\n", quad_nlp(fam, y, mu, s2, par));
    ++n;
  }
  fprintf(stderr, "%ld rows\n", n);
  return n > 0 ? 0 : 1;
}
