// smpc_own.h — the four holders of what the host side allocates: device memory, pinned host
// memory, events and streams.  Each owns one resource or none, moves (the source is left empty),
// does not copy, and frees what it holds when it goes.  Nothing else frees: a buffer that is
// declared as a holder cannot be forgotten by a teardown.  Internal: not part of the C-ABI.
//
// No exceptions: what can fail returns the runtime's hipError_t.  The file needs the runtime's
// declarations only, so a plain C++ compiler builds it (tests/own_check).
#ifndef SMPC_OWN_H_
#define SMPC_OWN_H_

#include <hip/hip_runtime_api.h>

// not part of the C-ABI: the members the compiler does not inline stay out of the dynamic symbol table
#pragma GCC visibility push(hidden)

namespace smpc_impl {

// Device memory: `capacity()` elements of T.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {o.p_ = nullptr; o.cap_ = 0;}
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() {reset();}
  T* get() const {return p_;}
  explicit operator bool() const {return p_ != nullptr;}
  size_t capacity() const {return cap_;}
  // Room for `count` elements: held already — nothing; empty or smaller — the old block is freed
  // and a new one allocated (its contents are NOT carried over).  After a failed allocation the
  // holder is empty, capacity 0.
  hipError_t ensure(size_t count)
  {
    if (p_ && cap_ >= count) return hipSuccess;
    reset();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    cap_ = count;
    return hipSuccess;
  }
  // a block allocated elsewhere that hipFree releases (fine-grained memory): the holder's from here on
  void adopt(T* p, size_t count)
  {
    reset();
    p_ = p; cap_ = count;
  }
  // the caller takes the block over
  T* release()
  {
    T* p = p_;
    p_ = nullptr; cap_ = 0;
    return p;
  }
  void reset()
  {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Pinned host memory (hipHostMalloc with the flags given): as DevBuf.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {o.p_ = nullptr; o.cap_ = 0;}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept
  {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~PinnedBuf() {reset();}
  T* get() const {return p_;}
  explicit operator bool() const {return p_ != nullptr;}
  size_t capacity() const {return cap_;}
  hipError_t ensure(size_t count, unsigned int flags = hipHostMallocDefault)
  {
    if (p_ && cap_ >= count) return hipSuccess;
    reset();
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, count * sizeof(T), flags);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    cap_ = count;
    return hipSuccess;
  }
  T* release()
  {
    T* p = p_;
    p_ = nullptr; cap_ = 0;
    return p;
  }
  void reset()
  {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr; cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// An event.  ensure(): created at the first call (hipEventDefault: what hipEventCreate makes),
// kept after that.
class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) {o.e_ = nullptr;}
  Event& operator=(Event&& o) noexcept
  {
    if (this != &o) {
      reset();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~Event() {reset();}
  hipEvent_t get() const {return e_;}
  explicit operator bool() const {return e_ != nullptr;}
  hipError_t ensure(unsigned int flags = hipEventDefault)
  {
    if (e_) return hipSuccess;
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) e_ = nullptr;
    return e;
  }
  hipEvent_t release()
  {
    hipEvent_t e = e_;
    e_ = nullptr;
    return e;
  }
  void reset()
  {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A stream: as Event.
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) {o.s_ = nullptr;}
  Stream& operator=(Stream&& o) noexcept
  {
    if (this != &o) {
      reset();
      s_ = o.s_;
      o.s_ = nullptr;
    }
    return *this;
  }
  ~Stream() {reset();}
  hipStream_t get() const {return s_;}
  explicit operator bool() const {return s_ != nullptr;}
  hipError_t ensure(unsigned int flags)
  {
    if (s_) return hipSuccess;
    const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
    if (e != hipSuccess) s_ = nullptr;
    return e;
  }
  hipStream_t release()
  {
    hipStream_t s = s_;
    s_ = nullptr;
    return s;
  }
  void reset()
  {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace smpc_impl

#pragma GCC visibility pop

#endif  // SMPC_OWN_H_
