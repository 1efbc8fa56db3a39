// tdsa_capi_mem.hpp - who owns memory in the C-ABI layer: Dev<T> a device buffer, Pinned<T> a pinned host block.  Each
// holds the pointer and its capacity in elements of T (byte buffers: Dev<char>), so that the two change together, is
// freed exactly once - by release() or by the destructor of whatever holds it, a half-built handle included - and
// cannot be copied.  Constructing one makes no HIP call.  Both convert to T*, so launch structs and copies take them
// as they took the raw pointers; as<U>() reads a byte buffer as the records it holds.  Included by
// tdsa_capi_internal.hpp, behind HIPCHK.  The only other hipMalloc / hipFree of the layer are those of caller-owned
// memory (tdsa_dev_alloc, tdsa_peer_alloc and their kin).
#pragma once

namespace tdsa {
#pragma GCC visibility push(hidden)

template <class T>
class Dev {
 public:
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() { release(); }

  // create chains (if (e == hipSuccess) e = ...) and the buffers made on first use: n elements, in place of what was held
  hipError_t alloc(size_t n) {
    release();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    if (e == hipSuccess) cap_ = n;
    return e;
  }
  // Buffers that grow on demand.  drain: the stream whose work may still use the old buffer, waited for before it is
  // freed (null: nobody can).  Synchronize, free, clear, allocate, record - in that order, so that a failed allocation
  // leaves an empty buffer of capacity 0.
  int grow(size_t need, hipStream_t drain) {
    if (need <= cap_) return TDSA_OK;
    if (drain) HIPCHK(hipStreamSynchronize(drain));
    if (p_) HIPCHK(hipFree(p_));
    p_ = nullptr;
    cap_ = 0;
    HIPCHK(alloc(need));
    return TDSA_OK;
  }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  template <class U>
  U* as() const { return reinterpret_cast<U*>(p_); }   // a byte buffer as what it holds
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// ... the same for pinned host memory; alloc and grow take the hipHostMalloc flags of their site
template <class T>
class Pinned {
 public:
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { release(); }

  hipError_t alloc(size_t n, unsigned flags) {
    release();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), flags);
    if (e == hipSuccess) cap_ = n;
    return e;
  }
  int grow(size_t need, hipStream_t drain, unsigned flags = hipHostMallocPortable | hipHostMallocMapped) {
    if (need <= cap_) return TDSA_OK;
    if (drain) HIPCHK(hipStreamSynchronize(drain));
    if (p_) HIPCHK(hipHostFree(p_));
    p_ = nullptr;
    cap_ = 0;
    HIPCHK(alloc(need, flags));
    return TDSA_OK;
  }
  void release() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  template <class U>
  U* as() const { return reinterpret_cast<U*>(p_); }   // a byte buffer as what it holds
  size_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

#pragma GCC visibility pop
}  // namespace tdsa
