// TEST-ONLY: the recombination with a small top word (city-rollup_amd/csrc/poseidon.h `recombine_s`, `repair_s`) at its three sites, and
// the partial rounds' b block in its triangular basis, as __host__ __device__ element bodies: the host library (recombine_hostsim.hip)
// calls them in a loop of one, the device library (recombine_devsim.hip) one element per lane. Never loaded by the product path.
#pragma once
#include "../../city-rollup_amd/csrc/gl.h"

namespace rsim {
// how often the rare path ran, per site (0 a full-round layer, 1 one partial round, 2 the exit of the partial rounds): host only
inline unsigned long long wrap_runs[3];
GL_HD void probe(int site) {
#if !defined(__HIP_DEVICE_COMPILE__)
  wrap_runs[site]++;
#else
  (void)site;
#endif
}
}  // namespace rsim
#define POSEIDON_WRAP_PROBE(site) rsim::probe(site)
#include "../../city-rollup_amd/csrc/poseidon.h"

namespace rsim {
using namespace poseidon;

// One site of `recombine_s` as the permutation runs it. site 0: the twelve of a full-round layer with the constants of round
// `idx` (30: none); site 1: the one of partial round `idx` (l[0], h[0] -> out[0]); site 2: the twelve of the exit of the partial
// rounds. Sites 1 and 2 take their limbs in the unit the planes are kept in (2^32 by default).
GL_HD void recombine_site(int site, int idx, const double *l, const double *h, uint64_t *out) {
  if (site == 1) {
    uint64_t r[1], wrap[1];
    r[0] = recombine_s<TOP0_PLANES>(l[0], h[0], doms_k(idx), wrap[0]);
    repair_s(r, wrap, 1);
    out[0] = r[0];
    return;
  }
  double yl[W], yh[W];
  uint64_t r[W];
#pragma unroll
  for (int k = 0; k < W; k++) yl[k] = l[k], yh[k] = h[k];
  if (site == 0) recombine_all_s<POSEIDON_TOP0_FULL>(yl, yh, [&](int k) { return rcs(idx >= 0 && idx < ROUNDS ? idx * W + k : ROUNDS * W); }, r, 0);
  else recombine_all_s<TOP0_PLANES>(yl, yh, [&](int k) { return doms_last(k); }, r, 2);
#pragma unroll
  for (int k = 0; k < W; k++) out[k] = r[k];
}
}  // namespace rsim
