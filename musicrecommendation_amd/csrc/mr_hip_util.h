// mr_hip_util.h — host scaffolding shared by the engine's .hip translation
// units: the error slot's declaration, the HIP call check, the scratch buffers
// of one call and the readers of diagnostic settings and model arguments.
// Includes the HIP runtime: the plain C++ units (mr_host.cpp, mr_modelio.cpp,
// mr_group.cpp) do not include it.
#ifndef MR_UTIL_HIP_H
#define MR_UTIL_HIP_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "mr_engine.h"

namespace mr_host {
int fail(int code, const char* fmt, ...);  // thread-local error slot (mr_engine.hip)
}

#define MR_HIP(call)                                                                                        \
  do {                                                                                                      \
    hipError_t e_ = (call);                                                                                 \
    if (e_ != hipSuccess)                                                                                   \
      return ::mr_host::fail(e_ == hipErrorOutOfMemory ? MR_E_OOM : MR_E_HIP, "%s failed: %s (%s:%d)", #call, \
                             hipGetErrorString(e_), __FILE__, __LINE__);                                    \
  } while (0)

namespace mr_hip {

template <typename T>
struct Tmp {  // scratch device buffer of one call, stream-ordered (pool allocator: no device sync)
  T* p = nullptr;
  hipStream_t st = nullptr;
  ~Tmp() { if (p) (void)hipFreeAsync(p, st); }
  int alloc(size_t n, hipStream_t s) {  // n elements, allocated and later freed on s
    st = s;
    MR_HIP(hipMallocAsync(reinterpret_cast<void**>(&p), n * sizeof(T), s));
    return MR_OK;
  }
};

struct Drain {  // the call's host tables outlive their copies on every return path
  hipStream_t st = nullptr;
  ~Drain() { (void)hipStreamSynchronize(st); }
};

// A diagnostic setting NAME=n clamped to [lo, hi]; hi when unset.
inline int env_clamped(const char* name, int lo, int hi) {
  const char* e = std::getenv(name);
  return e ? std::min(hi, std::max(lo, std::atoi(e))) : hi;
}

// The asymmetric models' alpha in [0, 1] and q in [1, MR_ASYM_MAX_Q].
inline int check_asym_args(double alpha, int q) {
  if (!(alpha >= 0.0 && alpha <= 1.0)) return mr_host::fail(MR_E_INVALID, "alpha=%g must be in [0,1]", alpha);
  if (q < 1 || q > MR_ASYM_MAX_Q) return mr_host::fail(MR_E_INVALID, "q=%d must be in [1,%d]", q, MR_ASYM_MAX_Q);
  return MR_OK;
}

}  // namespace mr_hip

#endif  // MR_UTIL_HIP_H
