// Permutations by lexicographic rank (the order of itertools.permutations), shared by the
// permutation searches of ctn_pit.hip and ctn_pitvar.hip.
#pragma once
#include "ctn_common.h"

namespace ctn {

// lexicographic rank of a permutation of range(C) (itertools.permutations order)
CTN_DEV long pit_rank(const int* perm, int C) {
  long r = 0, f = 1;
  for (int i = 2; i < C; ++i) f *= i;   // (C-1)!
  unsigned used = 0;
  for (int i = 0; i < C; ++i) {
    int smaller = 0;
    for (int v = 0; v < perm[i]; ++v) smaller += !((used >> v) & 1u);
    used |= 1u << perm[i];
    r += smaller * f;
    if (C - 1 - i > 0) f /= C - 1 - i;
  }
  return r;
}

// permutation of range(C) with lexicographic rank p (itertools.permutations order)
CTN_DEV void pit_decode(long p, int C, int* out) {
  long f = 1;
  for (int i = 2; i < C; ++i) f *= i;   // (C-1)!
  unsigned used = 0;
  for (int i = 0; i < C; ++i) {
    const int d = (int)(p / f);
    p %= f;
    if (C - 1 - i > 0) f /= C - 1 - i;
    int v = 0;
    for (int cnt = -1; v < C; ++v)
      if (!((used >> v) & 1u) && ++cnt == d) break;
    used |= 1u << v;
    out[i] = v;
  }
}

}  // namespace ctn
