// What the host side of libxmapper_hip.so stands on (included once, by xm_capi.hip): HIP error checking, the thread's last error of the C ABI,
// device buffers that own their memory, the pool of pinned host buffers the result streams live in.
#pragma once
#include "../../include/xmapper_hip.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

thread_local std::string g_error;
int fail(const std::string& msg) { g_error = msg; return 1; }

#define HIP_CHECK(expr)                                                                                     \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

// n elements of device memory, owned: freed by the destructor (on the device that is current then), moved but never copied
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  void ensure(size_t count) {
    if (count <= n && p) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = count ? count : 1;
    HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
  }
  // like ensure, but an allocation the GPU has no room for returns false (the buffer is then empty) instead of throwing
  bool tryEnsure(size_t count) {
    if (count <= n && p) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    const size_t want = count ? count : 1;
    n = 0;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) { (void)hipGetLastError(); p = nullptr; return false; }
    HIP_CHECK(e);
    n = want;
    return true;
  }
  // grow to `count`, keeping the first `keep` elements
  void growKeep(size_t count, size_t keep, hipStream_t s) {
    if (count <= n && p) return;
    T* np = nullptr;
    HIP_CHECK(hipMalloc((void**)&np, count * sizeof(T)));
    if (p && keep) HIP_CHECK(hipMemcpyAsync(np, p, (keep < n ? keep : n) * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (p) (void)hipFree(p);
    p = np; n = count;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  ~DevBuf() { release(); }
};

// The N timing events of a stage: created by the first call that records them (ready()), destroyed with their owner
template <int N>
struct StageEvents {
  hipEvent_t e[N] = {};
  StageEvents() = default;
  StageEvents(const StageEvents&) = delete;
  StageEvents& operator=(const StageEvents&) = delete;
  void ready() { for (hipEvent_t& x : e) if (!x) HIP_CHECK(hipEventCreate(&x)); }
  hipEvent_t operator[](int i) const { return e[i]; }
  ~StageEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// Result streams live in pinned host memory (the final device-to-host copy is then one DMA per stream); the buffers are recycled
// through a process-wide pool because pinning is far more expensive than the copy itself.
struct PinnedPool {
  struct Buf { void* p; size_t bytes; };
  std::mutex mu;
  std::vector<Buf> idle;
  size_t idleBytes = 0;
  std::atomic<size_t> allocatedBytes{0}, highWater{0};  // pinned host memory this process holds through the pool (in use + idle), and the most it ever held
  void account(long long delta) {
    const size_t now = (size_t)((long long)allocatedBytes.fetch_add((size_t)delta) + delta);
    size_t hw = highWater.load();
    while (now > hw && !highWater.compare_exchange_weak(hw, now)) {}
  }
  void* get(size_t bytes, size_t* got) {
    if (bytes < 64) bytes = 64;
    {
      std::lock_guard<std::mutex> lock(mu);
      int best = -1;
      for (int i = 0; i < (int)idle.size(); i++)
        if (idle[i].bytes >= bytes && idle[i].bytes <= bytes * 2 + 4096 && (best < 0 || idle[i].bytes < idle[best].bytes)) best = i;
      if (best >= 0) {
        Buf b = idle[best];
        idle.erase(idle.begin() + best);
        idleBytes -= b.bytes;
        *got = b.bytes;
        return b.p;
      }
    }
    void* p = nullptr;
    size_t want = bytes + bytes / 8;  // headroom so that the next, slightly larger batch reuses it
    HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocPortable));
    account((long long)want);
    *got = want;
    return p;
  }
  void put(void* p, size_t bytes) {
    if (!p) return;
    std::vector<Buf> drop;
    {
      std::lock_guard<std::mutex> lock(mu);
      idle.push_back(Buf{p, bytes});
      idleBytes += bytes;
      while (idleBytes > (4ull << 30) && !idle.empty()) {  // oldest first
        drop.push_back(idle.front());
        idleBytes -= idle.front().bytes;
        idle.erase(idle.begin());
      }
    }
    for (auto& b : drop) { (void)hipHostFree(b.p); account(-(long long)b.bytes); }
  }
};
static PinnedPool* g_pinned = new PinnedPool();  // never destroyed: the HIP runtime may be gone before static destructors run

// xm_result plus what xm_result_free needs to know about its buffers
struct ResultBox {
  xm_result pub;
  size_t bytesInts, bytesDbls, bytesIntOff, bytesDblOff;
};

}  // namespace
