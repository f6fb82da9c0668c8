// Leaf hash at the headline shape (2^20 leaves x 135 columns = 4096 workgroups of four waves) with a CHOSEN number of workgroups
// resident per CU: 16 wave-sized units per SIMD run as 5 + 5 + 5 + 1 with five resident, as 4 + 4 + 4 + 4 with four. Residency is
// set by the launch, not by the register count: every workgroup asks for so much dynamic LDS that exactly R fit the CU's 160 KB.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Icity-rollup_amd/csrc tools/ubench_leaf_residency.hip -o tools/ubench_leaf_residency
//   ... -DLEAF_RESIDENT=4 -o tools/ubench_leaf_residency_r4                                (register budget of four waves: 128)
//   ... -DLEAF_RESIDENT=4 -DPOSEIDON_INTERLEAVE_PLANES -o tools/ubench_leaf_residency_r4i  (and the two planes of dom_mul2_d interleaved)
//   ... -DLEAF_FUSE=1 ...                                                                   (with fused levels, merkle.h fused_levels)
// Prints, per R: the code object's registers and static LDS, the dynamic LDS asked for, the residency the runtime derives from
// them, ms per launch (median and minimum of 7 timed groups of 5 launches) and a checksum of the digests (the same in every row).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "merkle.h"
#include "poseidon_tables.h"

#ifndef LEAF_RESIDENT
#define LEAF_RESIDENT 5
#endif
#ifndef LEAF_FUSE
#define LEAF_FUSE 0
#endif
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

int main() {
  CK(hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_RC), POSEIDON_RC, sizeof POSEIDON_RC));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_RCD), POSEIDON_RCD, sizeof POSEIDON_RCD));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_DDK), poseidon::DDK_HOST, sizeof poseidon::DDK_HOST));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_DDLAST), poseidon::DDLAST_HOST, sizeof poseidon::DDLAST_HOST));
  const int k = 135, log_n = 20;
  const size_t n = (size_t)1 << log_n;
  auto kern = merkle::k_leaf_hash_cols<false, LEAF_FUSE, LEAF_RESIDENT>;
  hipFuncAttributes fa;
  CK(hipFuncGetAttributes(&fa, (const void *)kern));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const size_t lds_cu = std::max(prop.maxSharedMemoryPerMultiProcessor, prop.sharedMemPerBlock);  // 160 KB on gfx950
  printf("LDS per CU %zu B\n", lds_cu);
  printf("kernel k_leaf_hash_cols<false, %d, %d>%s: %d registers, %zu B static LDS, %zu B scratch; %d CUs\n", LEAF_FUSE, LEAF_RESIDENT,
#if defined(POSEIDON_INTERLEAVE_PLANES)
         " planes interleaved",
#else
         "",
#endif
         fa.numRegs, fa.sharedSizeBytes, fa.localSizeBytes, prop.multiProcessorCount);
  std::vector<uint64_t> h(n * k);
  uint64_t x = 0x243F6A8885A308D3ull;
  for (auto &v : h) { x += 0x9E3779B97F4A7C15ull; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31; v = z % gl::P; }
  uint64_t *d_cols, *d_dig;
  CK(hipMalloc(&d_cols, n * k * 8));
  CK(hipMalloc(&d_dig, 2 * n * 32));  // every level fits
  CK(hipMemcpy(d_cols, h.data(), n * k * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const dim3 grid((unsigned)(n / merkle::THREADS), 1), block(merkle::THREADS);
  for (int R = 3; R <= LEAF_RESIDENT; R++) {
    // R workgroups fit, R + 1 do not: R (dyn + static) <= LDS of a CU < (R + 1) (dyn + static), in every row
    size_t dyn = (lds_cu / R - fa.sharedSizeBytes) & ~(size_t)1023;
    if ((R + 1) * (dyn + fa.sharedSizeBytes) <= lds_cu || R * (dyn + fa.sharedSizeBytes) > lds_cu) { printf("R = %d: no LDS size caps it\n", R); return 1; }
    CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    int resident = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, merkle::THREADS, dyn));
    if (resident != R) { printf("R = %d asked, the runtime derives %d from %d registers and %zu B LDS: not measured\n", R, resident, fa.numRegs, dyn + fa.sharedSizeBytes); continue; }
    auto launch = [&]() { hipLaunchKernelGGL(kern, grid, block, dyn, 0, d_cols, n, k, n, d_dig, (size_t)0, (size_t)0, nullptr, 0, (size_t)0); };
    for (int w = 0; w < 3; w++) launch();
    CK(hipDeviceSynchronize());
    std::vector<float> t;
    for (int g = 0; g < 7; g++) {
      CK(hipEventRecord(e0));
      for (int r = 0; r < 5; r++) launch();
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      t.push_back(ms / 5);
    }
    std::sort(t.begin(), t.end());
    std::vector<uint64_t> dig(n * 4);
    CK(hipMemcpy(dig.data(), d_dig, n * 32, hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (auto v : dig) sum = sum * 0x100000001B3ull + v;
    printf("R = %d resident workgroups per CU (dynamic LDS %zu B): %.4f ms per launch median, %.4f min, %.4f max  leaf digest checksum %016llx\n", R, dyn,
           t[3], t[0], t[6], (unsigned long long)sum);
  }
  return 0;
}
