// devbuf.hpp -- the owners of device resources: a buffer, an event, a stream.  Each frees what it holds in its destructor and
// can be moved but not copied, so a function may return wherever it likes and a struct of them needs no clean-up code.
// Host-only: HIP's runtime API and standard headers, nothing else.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <utility>

template <typename T> struct DevBuf
{
  T *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    if(this != &o)
      {
        release();
        p = std::exchange(o.p, nullptr);
        cap = std::exchange(o.cap, 0);
      }
    return *this;
  }
  ~DevBuf() { release(); }
  // room for n elements; a grow does not keep the contents.  -1: out of memory, and the buffer is empty
  int ensure(size_t n)
  {
    if(n <= cap)
      return 0;
    release();
    size_t want = n + n / 16 + 64;
    if(hipMalloc((void **)&p, want * sizeof(T)) != hipSuccess)
      {
        p = nullptr;
        return -1;
      }
    cap = want;
    return 0;
  }
  void release()
  {
    if(p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// One handle H made by Create and destroyed by Destroy; converts to H, so that launches, records and waits take it as they take
// the handle itself
template <typename H, hipError_t (*Create)(H *), hipError_t (*Destroy)(H)> struct DevHandle
{
  H h = nullptr;
  DevHandle() = default;
  DevHandle(const DevHandle &) = delete;
  DevHandle &operator=(const DevHandle &) = delete;
  DevHandle(DevHandle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
  DevHandle &operator=(DevHandle &&o) noexcept
  {
    if(this != &o)
      adopt(std::exchange(o.h, nullptr));
    return *this;
  }
  ~DevHandle() { adopt(nullptr); }
  hipError_t create()
  {
    adopt(nullptr);
    const hipError_t e = Create(&h);
    if(e != hipSuccess)
      h = nullptr;
    return e;
  }
  // owns `x` from now on (a stream that hipExtStreamCreateWithCUMask made, say); what it held before is destroyed
  void adopt(H x)
  {
    if(h)
      (void)Destroy(h);
    h = x;
  }
  operator H() const { return h; }
};
using DevEvent = DevHandle<hipEvent_t, hipEventCreate, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamCreate, hipStreamDestroy>;
