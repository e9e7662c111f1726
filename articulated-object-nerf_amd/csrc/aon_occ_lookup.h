// The occupancy lookup of DESIGN.md section 4.9, used by aon_occ.hip's one mark / emit pair for every path (one grid per render, sections 4.9 - 4.11;
// one grid per placed object, section 4.17): sample x lies in cell floor((x_a - lo_a) / step_a) per axis (fp32 subtraction, IEEE division, floor), clamped to cells_a - 1
// (x_a == hi_a); a coordinate outside [lo_a, hi_a], or NaN, is EMPTY.  tests/_occ_ref.py is an independent numpy copy.
#pragma once
#include "aon_common.h"

namespace aon {

__device__ __forceinline__ bool occ_lookup(const OccGrid& G, const float (&x)[3]) {
  int64_t c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(x[a] >= G.lo[a] && x[a] <= G.hi[a])) return false;   // outside the box, or NaN
    const int64_t q = (int64_t)__builtin_floorf(__fdiv_rn(__fsub_rn(x[a], G.lo[a]), G.step[a]));
    c[a] = q < G.cells[a] - 1 ? q : G.cells[a] - 1;
  }
  const int64_t lin = (c[0] * G.cells[1] + c[1]) * G.cells[2] + c[2];
  return (G.bits[lin >> 5] >> (lin & 31)) & 1u;
}

}  // namespace aon
