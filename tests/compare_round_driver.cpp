/* Answers aad_compare_round.h's questions for the rows on stdin, one line each (tests/test_compare_round.py).
 *   n v        (n: value count, decimal; v: a double in C99 hex-float form)
 *     -> rel crosses   (rel = compare_reorder_bound(n) in hex-float form; crosses = compare_crosses_boundary(v, rel), 0 / 1) */
#include <cstdio>
#include <cstdlib>

#include "aad_compare_round.h"

int main()
{
  char n_text[64], v_text[64];
  while (scanf("%63s %63s", n_text, v_text) == 2) {
    const double n = (double)strtoull(n_text, nullptr, 10), v = strtod(v_text, nullptr);
    const double rel = aad::compare_reorder_bound(n);
    printf("%a %d\n", rel, aad::compare_crosses_boundary(v, rel) ? 1 : 0);
  }
  return 0;
}
