// The Groth16 key handle: made by the setup (groth16_setup.inc, in bls.hip) and by the loader of key files (keyfile.hip),
// read by both and by cp_groth16_key_pk / cp_groth16_key_vk. Host-only.
#pragma once
#include "core.h"

struct cp_groth16_key {
  explicit cp_groth16_key(int dev) : device(dev), mem(dev_pool(), dev) {}
  const int device;
  cp_groth16_pk pk{};
  cp_groth16_vk vk{};
  std::vector<uint64_t> ic_xy;  // n_public x 12
  std::vector<uint8_t> ic_inf;
  DevBag mem;  // the five point sets and the two flag arrays
};

namespace {

void groth16_key_free(cp_groth16_key *k) {
  if (!k) return;
  if (k->mem.size()) (void)hipSetDevice(k->device);
  delete k;
}

}  // namespace
