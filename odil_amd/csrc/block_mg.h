// The level representation of the normal-equation multigrid (block_mg.hip), shared with the coarsest-level
// factorisation (coarse_chol.hip).
#pragma once
#include "common.h"

namespace odil {

constexpr int kBmgMaxFields = 8;
constexpr int kEnt = 8;  // int64 words per table entry: a, b, o0, o1, o2, start, (unused) x2

struct BmgLevel {
  int nf;
  int64_t off[kBmgMaxFields + 1];
  int64_t n[kBmgMaxFields][3];
  int ebeg[kBmgMaxFields + 1];
};

// desc: nf, off[0..nf], n[f][0..2] for f < nf, ebeg[0..nf]
static int parse_level(const int64_t* desc, BmgLevel& L, const char* what) {
  if (!desc || desc[0] < 1 || desc[0] > kBmgMaxFields) {
    set_error("%s: invalid level descriptor (1 to %d fields)", what, kBmgMaxFields);
    return ODIL_E_INVAL;
  }
  memset(&L, 0, sizeof(L));
  L.nf = (int)desc[0];
  const int64_t* p = desc + 1;
  for (int f = 0; f <= L.nf; ++f) L.off[f] = *p++;
  for (int f = 0; f < L.nf; ++f)
    for (int d = 0; d < 3; ++d) {
      L.n[f][d] = *p++;
      if (L.n[f][d] < 1) {
        set_error("%s: empty extent", what);
        return ODIL_E_INVAL;
      }
    }
  for (int f = 0; f <= L.nf; ++f) L.ebeg[f] = (int)*p++;
  for (int f = 0; f < L.nf; ++f)
    if (L.off[f + 1] - L.off[f] != L.n[f][0] * L.n[f][1] * L.n[f][2] || L.ebeg[f + 1] < L.ebeg[f]) {
      set_error("%s: field offsets do not match the shapes", what);
      return ODIL_E_INVAL;
    }
  return 0;
}

__device__ inline int field_of(const BmgLevel& L, int64_t i) {
  int f = 0;
  while (f + 1 < L.nf && i >= L.off[f + 1]) ++f;
  return f;
}

}  // namespace odil
