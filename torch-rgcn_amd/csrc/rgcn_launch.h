// Host-side launch state, kept PER DEVICE: the compute-unit count that sizes persistent grids, and which kernels may already use more
// than 64 KiB of dynamic LDS.  hipFuncSetAttribute applies to the current device only, and autograd runs backward on one thread per
// device -- so the state is indexed by device id and written with relaxed atomics (a second writer stores the same value).
// Everything here is internal to its translation unit (anonymous namespace): the C ABI does not see it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

namespace {

constexpr int LAUNCH_DEVS = 32;      // device ids with remembered state (one bit each in allow_lds); an id outside asks the runtime every time

// The current device and its compute-unit count (256 when the runtime reports none).
inline hipError_t launch_device(int *dev, int *n_cu) {
  static std::atomic<int> cus[LAUNCH_DEVS];
  hipError_t e = hipGetDevice(dev);
  if (e != hipSuccess) return e;
  const bool slot = (unsigned)*dev < (unsigned)LAUNCH_DEVS;
  int v = slot ? cus[*dev].load(std::memory_order_relaxed) : 0;
  if (!v) {
    e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, *dev);
    if (e != hipSuccess) return e;
    v = v > 0 ? v : 256;
    if (slot) cus[*dev].store(v, std::memory_order_relaxed);
  }
  *n_cu = v;
  return hipSuccess;
}

// A kernel as a value whose TYPE names it, so that a generic launch lambda can hand it on as a template argument:
//   launch(kern_c<my_kernel<true, 2>>)  ...  [&](auto k) { constexpr auto kern = decltype(k)::value; allow_lds<kern>(dev, lds, MAX); ... }
template <auto Kern>
constexpr std::integral_constant<decltype(Kern), Kern> kern_c{};

// Allow Kern up to max_bytes of dynamic LDS on device `dev` when this launch needs more than the 64 KiB every kernel may use: one
// hipFuncSetAttribute per kernel and device (the static is per instantiation), none after the first launch on a device.  Not a stream
// operation: warm-up launches keep it out of captured graphs.
template <auto Kern>
hipError_t allow_lds(int dev, size_t need, int max_bytes) {
  static std::atomic<unsigned> done{0u};
  if (need <= 64 * 1024) return hipSuccess;
  const unsigned bit = (unsigned)dev < (unsigned)LAUNCH_DEVS ? 1u << dev : 0u;
  if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
  return e;
}

}  // namespace
