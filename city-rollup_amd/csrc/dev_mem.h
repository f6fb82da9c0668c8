// Owners of device (and page-locked host) memory, over the pool type so that the logic can be unit-tested on the CPU
// (tests/hostsim: DevPoolT over a counting allocator). The product instantiates them on dev_pool() (core.h). Host-only.
//
// DevBufT owns ONE buffer: pointer, byte count, device. It is move-only and has exactly two ways of giving the buffer back,
// fixed when the owner is made:
//   RUNTIME  obtained through pool.malloc, given back through the raw free (which waits for the device).
//   POOLED   obtained through pool.alloc, given back through pool.release(device, p, bytes, reusable). `reusable` is true
//            only if the owner was TOLD the buffer is idle: by mark_idle(), or by the stream-idle callback given at
//            construction (the product: hipStreamSynchronize(ctx->stream) == hipSuccess), asked when the buffer is given
//            back. mark_exported() (the pointer left the library) or an owner that cannot establish idleness releases
//            non-reusable: the runtime free. Only idle buffers enter the pool (dev_pool.h); nothing else can put one there.
// grow(bytes) is the grow-only buffer: too small -> wait through the callback, give the old buffer back, allocate the new
// size; the owner is empty (size 0) if that allocation fails. DevBagT is "every temporary of this call": when it dies with
// buffers in it, it asks the callback ONCE and gives all of them back under that answer - the trailing synchronisation a
// temporary needs when work on it may still be queued.
//
// Rules:
//  1. Destroying an owner assumes nothing about the current device beyond what the raw free needs.
//  2. cp_ctx_destroy synchronises the stream before any owner of the context is cleared and destroys the stream after the
//     last of them; it does so in explicit statements, not through the declaration order of the members.
#pragma once
#include <cstddef>
#include <functional>
#include <utility>
#include <vector>

enum class DevOwn { RUNTIME, POOLED };

template <class Pool>
class DevBufT {
 public:
  using Idle = std::function<bool()>;

  DevBufT() = default;  // unbound: holds nothing and can only be assigned to
  DevBufT(Pool &pool, int device, DevOwn own = DevOwn::RUNTIME, Idle idle = {}) : pool_(&pool), device_(device), own_(own), idle_(std::move(idle)) {}
  DevBufT(DevBufT &&o) noexcept { *this = std::move(o); }
  DevBufT &operator=(DevBufT &&o) noexcept {
    if (this != &o) {
      reset();
      pool_ = o.pool_; device_ = o.device_; own_ = o.own_; idle_ = std::move(o.idle_); state_ = o.state_; bytes_ = o.bytes_;
      p_ = o.release();
    }
    return *this;
  }
  DevBufT(const DevBufT &) = delete;
  DevBufT &operator=(const DevBufT &) = delete;
  ~DevBufT() { reset(); }

  // gives back what it holds, then allocates; returns the pool's status (0 = ok), the owner empty on failure
  int alloc(size_t bytes) {
    reset();
    void *p = nullptr;
    const int e = own_ == DevOwn::POOLED ? pool_->alloc(device_, &p, bytes) : pool_->malloc(device_, &p, bytes);
    if (e == 0) { p_ = p; bytes_ = bytes; state_ = ASK; }
    return e;
  }
  int grow(size_t bytes) {
    if (bytes_ >= bytes) return 0;
    if (p_ && idle_) idle_() ? mark_idle() : mark_exported();  // queued work may still use the old buffer
    return alloc(bytes);
  }
  void reset() {
    if (!p_) return;
    if (own_ == DevOwn::POOLED) pool_->release(device_, p_, bytes_, state_ == IDLE || (state_ == ASK && idle_ && idle_()));
    else Pool::free(p_);
    (void)release();
  }
  void *release() { void *p = p_; p_ = nullptr; bytes_ = 0; return p; }  // the caller owns the buffer from here on
  void mark_idle() { if (state_ != EXPORTED) state_ = IDLE; }  // no stream of the library can still be using the buffer
  void mark_exported() { state_ = EXPORTED; }                  // never reusable whatever is said later, and nobody is asked
  template <class T = void> T *get() const { return (T *)p_; }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  enum State { ASK, IDLE, EXPORTED };
  Pool *pool_ = nullptr;
  int device_ = -1;
  DevOwn own_ = DevOwn::RUNTIME;
  Idle idle_;
  State state_ = ASK;
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

template <class Pool>
class DevBagT {
 public:
  using Buf = DevBufT<Pool>;
  DevBagT(Pool &pool, int device, DevOwn own = DevOwn::RUNTIME, typename Buf::Idle idle = {}) : pool_(&pool), device_(device), own_(own), idle_(std::move(idle)) {}
  DevBagT(const DevBagT &) = delete;
  DevBagT &operator=(const DevBagT &) = delete;
  ~DevBagT() { clear(); }
  // allocates, appends and stores the typed pointer (nullptr on failure); returns the pool's status
  template <class T>
  int alloc(T **out, size_t bytes) {
    *out = nullptr;
    bufs_.reserve(bufs_.size() + 1);  // a bad_alloc cannot strand a buffer
    Buf b(*pool_, device_, own_);
    const int e = b.alloc(bytes);
    if (e) return e;
    *out = b.template get<T>();
    bufs_.push_back(std::move(b));
    return 0;
  }
  void clear() {
    if (bufs_.empty()) return;
    const bool idle = idle_ && idle_();
    for (Buf &b : bufs_) idle ? b.mark_idle() : b.mark_exported();
    bufs_.clear();
  }
  size_t size() const { return bufs_.size(); }

 private:
  Pool *pool_;
  int device_;
  DevOwn own_;
  typename Buf::Idle idle_;
  std::vector<Buf> bufs_;
};
