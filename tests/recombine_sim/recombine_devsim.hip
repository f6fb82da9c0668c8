// TEST-ONLY: the device form of `recombine_s` / `repair_s` (carry-outs in SGPR pairs, ORed and tested once, repaired behind one
// wave-uniform branch) on arrays the caller chooses, one element per lane, so that a test decides which lanes of a wave wrap.
// Built with the product's flags (recombine_sim_build.py). Never loaded by the product path.
#include "recombine_sim.h"

#include <hip/hip_runtime.h>

namespace {
constexpr int WG = 256;
__global__ __launch_bounds__(WG) void k_site(int site, int idx, const double *l, const double *h, uint64_t *out, size_t n) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  double ll[12], hh[12];
  uint64_t r[12];
  const int cnt = site == 1 ? 1 : 12;
  for (int k = 0; k < 12; k++) ll[k] = l[12 * i + k], hh[k] = h[12 * i + k], r[k] = out[12 * i + k];
  rsim::recombine_site(site, idx, ll, hh, r);
  for (int k = 0; k < cnt; k++) out[12 * i + k] = r[k];
}
}  // namespace

extern "C" {
// n elements of one site (rsim::recombine_site) on the device: l, h n x 12 doubles, out n x 12 (site 1 reads and writes [0] of each
// row and leaves the rest as the caller set it). Returns a hipError_t.
int rsd_site(int site, int idx, const double *l, const double *h, uint64_t *out, size_t n) {
  if (site < 0 || site > 2 || n == 0) return -1;
  double *dl = nullptr, *dh = nullptr;
  uint64_t *dout = nullptr;
  const size_t bytes = n * 12 * 8;
  int err = hipMalloc(&dl, bytes);
  if (!err) err = hipMalloc(&dh, bytes);
  if (!err) err = hipMalloc(&dout, bytes);
  if (!err) err = hipMemcpy(dl, l, bytes, hipMemcpyHostToDevice);
  if (!err) err = hipMemcpy(dh, h, bytes, hipMemcpyHostToDevice);
  if (!err) err = hipMemcpy(dout, out, bytes, hipMemcpyHostToDevice);
  if (!err) {
    k_site<<<(unsigned)((n + WG - 1) / WG), WG>>>(site, idx, dl, dh, dout, n);
    err = hipGetLastError();
  }
  if (!err) err = hipDeviceSynchronize();
  if (!err) err = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dl), (void)hipFree(dh), (void)hipFree(dout);
  return err;
}
}
