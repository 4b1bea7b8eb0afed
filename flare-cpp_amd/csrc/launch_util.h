// launch_util.h -- host-side helpers shared by the launch functions: stream
// ordering through a temporary event, and per-device lazily created stream /
// event sets.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>

namespace fsg {

// Orders `stream` behind whatever is queued on `pass1_stream` with a
// temporary event (two-stream calls whose passes all run on `stream`: no
// per-device event set, or a single-pass kernel).
inline hipError_t order_after(hipStream_t stream, hipStream_t pass1_stream) {
  hipEvent_t ev = nullptr;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ev, pass1_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(stream, ev, 0);
  if (ev) (void)hipEventDestroy(ev);
  return e;
}

// The current device's T, created on first use by create(T*) (once per
// device; false = its streams and events could not be created).  nullptr
// when creation failed or the device is unknown: the caller then runs in one
// stream.  T carries a mutex that orders each call's record/wait pairs when
// several host threads launch at once.
template <class T>
T* per_device(bool (*create)(T*)) {
  constexpr int kMaxDevices = 64;
  static T g[kMaxDevices];
  static bool ok[kMaxDevices];
  static std::once_flag once[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  std::call_once(once[dev], [&] { ok[dev] = create(&g[dev]); });
  return ok[dev] ? &g[dev] : nullptr;
}

}  // namespace fsg
