// TEST-ONLY: what every device twin (`ds_*`) of a hostsim wrapper is made of. A `Job` copies host arrays to the device, launches
// one element-wise kernel under a per-element mask and copies the outputs back. The primitive runs inside `if (mask[i])`, so
// EXEC is partial wherever the mask says so; an output the mask switches off keeps what the caller put there (a sentinel).
// Every launch has at least two workgroups of 256; every index is below the element count passed in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace devsim {

constexpr int WG = 256;

template <class F>
__global__ __launch_bounds__(WG) void k_each(const uint8_t *mask, size_t n, F f) {
  const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  if (mask[i]) f(i);
}

int unit_init();  // uploads the unit's __constant__ tables once; a hipError_t

class Job {
 public:
  Job(const uint8_t *mask, size_t n) : n_(n) {
    err_ = unit_init();
    mask_ = in(mask, n);
  }
  ~Job() {
    for (auto &b : bufs_) (void)hipFree(b.dev);
  }
  Job(const Job &) = delete;
  Job &operator=(const Job &) = delete;
  // `count` elements of T: read-only input / in-out (copied to the device, and back after the kernel)
  template <class T> const T *in(const T *host, size_t count) { return (const T *)add((void *)host, count * sizeof(T), false); }
  template <class T> T *inout(T *host, size_t count) { return (T *)add(host, count * sizeof(T), true); }
  template <class F> int run(F f) {
    if (err_) return err_;
    const unsigned blocks = (unsigned)((n_ + WG - 1) / WG);
    k_each<<<blocks < 2 ? 2 : blocks, WG>>>(mask_, n_, f);
    if ((err_ = hipGetLastError())) return err_;
    if ((err_ = hipDeviceSynchronize())) return err_;
    for (auto &b : bufs_)
      if (b.back && !err_) err_ = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost);
    return err_;
  }

 private:
  struct Buf { void *host, *dev; size_t bytes; bool back; };
  void *add(void *host, size_t bytes, bool back) {
    void *d = nullptr;
    if (err_) return nullptr;
    if ((err_ = hipMalloc(&d, bytes ? bytes : 8))) return nullptr;
    bufs_.push_back({host, d, bytes, back});
    if (bytes) err_ = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  size_t n_;
  int err_ = 0;
  const uint8_t *mask_ = nullptr;
  std::vector<Buf> bufs_;
};

}  // namespace devsim

// The body of a wrapper kernel. always_inline: a body the compiler leaves out of line becomes a FUNCTION with its return address in
// s[30:31], and in a function longer than the reach of s_branch (128 KiB: six permutation forms in one body were 315 KiB) the
// long-branch expansion of this compiler scratches exactly that pair: the return then jumps back into the body for ever.
// Inlined into the kernel there is no return address; and a kernel holds one form of a large primitive, as the product's do.
#define DS_EACH [=] __device__(size_t i) __attribute__((always_inline))
